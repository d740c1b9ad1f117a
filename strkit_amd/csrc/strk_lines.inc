// strk_lines.inc — the lines of the text in a strk_dbam object's stream (part of strk_api.hip, after strk_dbam.inc): the launches
// of strk_lines.h's kernels (dbam_lines), what the text readers built on it share (text_check, dbam_query), and the entry point
// that hands the line starts out as they are (strk_dbam_text_lines).  strk_vcf.inc and strk_gff.inc are the readers.

namespace {

// the arguments every text reader has, checked before anything is read
int text_check(const char* who, int64_t n_bytes, int64_t start, const char* contig, const void* size_out, const int64_t* end_off, const int32_t* past) {
    if (!contig || !contig[0]) return fail(STRK_E_INVALID, "%s: no contig name", who);
    if (!size_out || !end_off || !past) return fail(STRK_E_INVALID, "%s: NULL argument", who);
    if (n_bytes < 0 || start < 0 || start > n_bytes) return fail(STRK_E_INVALID, "%s: start offset %lld outside the text of %lld bytes", who, (long long)start, (long long)n_bytes);
    if (n_bytes - start >= ((int64_t)1 << 31)) return fail(STRK_E_INVALID, "%s: a piece of %lld bytes (at most 2^31 - 1)", who, (long long)(n_bytes - start));
    return 0;
}

struct DevLines {
    int64_t* starts = nullptr;   // device, [n_nl + 1] (ln_starts); NULL when start == n
    int32_t n_nl = 0, n_lines = 0;
    int64_t end_off = 0;
    dim3 line_grid;              // one lane per line, 256 a block
};

// The lines of data[start, n_data): the tile-size rule first (tile_bytes 0 = strk_lines::kTileBytes), then, unless start == n_data
// (nothing launched, *out as initialised with end_off = start), count | scan | one word back | scatter | one word back.
// ln_tiles: counts | offsets per tile; ln_starts: the line starts.
int dbam_lines(strk_dbam* d, const char* who, int64_t start, int32_t final, int32_t tile_bytes, DevLines* out) {
    if (tile_bytes == 0) tile_bytes = strk_lines::kTileBytes;
    if (!strk_lines::tile_bytes_ok(tile_bytes)) return fail(STRK_E_INVALID, "%s: tile_bytes must be a multiple of %d", who, strk_lines::kStepBytes);
    const int64_t n = d->n_data;
    *out = DevLines();
    out->end_off = start;
    if (start == n) return 0;
    HIP_TRY(hipSetDevice(d->device));
    const uint8_t* const data = d->data.as<uint8_t>();
    const int64_t t0 = start & ~(int64_t)(strk_lines::kStepBytes - 1);
    const int32_t n_tiles = (int32_t)((n - t0 + tile_bytes - 1) / tile_bytes);
    Carve ct;
    const size_t o_cnt = ct.take((size_t)n_tiles * 4), o_off = ct.take(((size_t)n_tiles + 1) * 8);
    int rc = d->ln_tiles.ensure(ct.bytes);
    if (rc) return rc;
    const dim3 tile_grid((unsigned)((n_tiles + 3) / 4));
    d->tic();
    hipLaunchKernelGGL(strk_lines::k_lines_count, tile_grid, dim3(256), 0, 0, data, n, start, tile_bytes, n_tiles, d->ln_tiles.at<int32_t>(o_cnt));
    hipLaunchKernelGGL(strk_lines::k_lines_scan, dim3(1), dim3(256), 0, 0, d->ln_tiles.at<int32_t>(o_cnt), n_tiles, d->ln_tiles.at<int64_t>(o_off));
    HIP_TRY(hipGetLastError());
    d->toc();
    int64_t n_nl64 = 0;
    HIP_TRY(hipMemcpy(&n_nl64, d->ln_tiles.at<int64_t>(o_off) + n_tiles, 8, hipMemcpyDeviceToHost));
    if (n_nl64 < 0 || n_nl64 > n - start) return fail(STRK_E_DEVICE, "%s: line count %lld out of range", who, (long long)n_nl64);
    const int32_t n_nl = (int32_t)n_nl64;
    const size_t cap_lines = (size_t)n_nl + 1;
    if ((rc = d->ln_starts.ensure(cap_lines * 8))) return rc;
    int64_t* const starts = d->ln_starts.as<int64_t>();
    d->tic();
    hipLaunchKernelGGL(strk_lines::k_lines_starts, tile_grid, dim3(256), 0, 0, data, n, start, tile_bytes, n_tiles, d->ln_tiles.at<int64_t>(o_off),
                       (int64_t)cap_lines, starts);
    HIP_TRY(hipGetLastError());
    d->toc();
    int64_t last_start = 0;
    HIP_TRY(hipMemcpy(&last_start, starts + n_nl, 8, hipMemcpyDeviceToHost));
    if (last_start < start || last_start > n) return fail(STRK_E_DEVICE, "%s: line start %lld out of range", who, (long long)last_start);
    out->starts = starts;
    out->n_nl = n_nl;
    out->n_lines = n_nl + ((final && last_start < n) ? 1 : 0);
    out->end_off = out->n_lines > n_nl ? n : last_start;
    out->line_grid = dim3((unsigned)((out->n_lines + 255) / 256));
    return 0;
}

// The four status words a reader's kernels fold into (with the reader's initial values) and the contig's name, on the device.
// ln_query: status words | name
int dbam_query(strk_dbam* d, const unsigned long long (&st0)[4], const char* contig, int32_t contig_len, unsigned long long** st, const uint8_t** name) {
    Carve cq;
    const size_t o_st = cq.take(32), o_name = cq.take((size_t)contig_len);
    const int rc = d->ln_query.ensure(cq.bytes);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(d->ln_query.at<char>(o_st), st0, 32, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d->ln_query.at<char>(o_name), contig, (size_t)contig_len, hipMemcpyHostToDevice));
    *st = d->ln_query.at<unsigned long long>(o_st);
    *name = d->ln_query.at<uint8_t>(o_name);
    return 0;
}

}  // namespace

extern "C" {

int64_t strk_dbam_text_lines(strk_dbam* d, int64_t start, int32_t final, int32_t tile_bytes, int64_t cap, int64_t* starts, int64_t* end_off,
                             int64_t* n_starts) {
    static const char who[] = "strk_dbam_text_lines";
    if (!d || !end_off || !n_starts || cap < 0 || (cap > 0 && !starts)) return fail(STRK_E_INVALID, "%s: bad argument", who);
    if (start < 0 || start > d->n_data) return fail(STRK_E_INVALID, "%s: start offset %lld outside the text of %lld bytes", who, (long long)start, (long long)d->n_data);
    if (d->n_data - start >= ((int64_t)1 << 31)) return fail(STRK_E_INVALID, "%s: a piece of %lld bytes (at most 2^31 - 1)", who, (long long)(d->n_data - start));
    DevLines l;
    const int rc = dbam_lines(d, who, start, final, tile_bytes, &l);
    if (rc) return rc;
    *end_off = l.end_off;
    *n_starts = (int64_t)l.n_nl + 1;
    const int64_t n_out = std::min(cap, *n_starts);
    if (!l.starts) {   // start == n_data: the one start there is
        if (n_out > 0) starts[0] = start;
    } else if (n_out > 0) {
        HIP_TRY(hipMemcpy(starts, l.starts, (size_t)n_out * 8, hipMemcpyDeviceToHost));
    }
    return l.n_lines;
}

}  // extern "C"
