// strk_dbam.inc — alignment file on the device (part of strk_api.hip): BGZF inflation, record scan and read extraction as
// HIP kernels, so that an alignment file goes from its compressed bytes to the CSR batch strk_submit_loci_device takes
// without its decompressed form (6x the file: gigabytes) ever crossing PCIe or a host core.
//
// Reference: the reader strkit_rust_ext wraps around htslib (STRkitBAMReader; call sites strkit/call/call_sample.py:103-121,
// strkit/call/call_locus.py:837-958) — not in the tree.  The rules are the ones strk_frontend.h / frontend/extract.py state
// and tests/test_frontend.py pins; the kernels here are checked against those host functions record by record.
//
// Layout in HBM: `comp` = the compressed stretch (padded by 16 bytes), `data` = the decompressed stream, contiguous in file
// order, `blocks` = one 32-byte descriptor per BGZF block.  One lane inflates one block (strk_inflate.h); 64-lane workgroups,
// 22 KB of LDS each (the lanes' symbol tables of 320 bytes, the CRC tables) -> seven workgroups per CU; the CRC of every block is checked by the lane that
// wrote it (slice-by-4 over a table in LDS), while its 64 KB are still in L2.

namespace {

struct InfBlock {
    int64_t in_off;    // offset of the deflate payload in `comp`
    int64_t out_off;   // offset of the block's bytes in `data`
    int32_t in_len;
    int32_t out_len;
    uint32_t crc;
    int32_t pad;
};

__global__ void __launch_bounds__(64) k_bgzf_inflate(const uint8_t* comp, const InfBlock* blocks, int n_blocks, uint8_t* data,
                                                     uint8_t* lens_scratch, unsigned long long* status) {
    __shared__ strk_inf::Tables tabs[64];
    __shared__ uint32_t crc_tab[2][256];
    for (int i = threadIdx.x; i < 256; i += 64) strk_inf::crc_table_entry(crc_tab[0], i);
    __syncthreads();
    for (int i = threadIdx.x; i < 256; i += 64) crc_tab[1][i] = crc_tab[0][crc_tab[0][i] & 0xffu] ^ (crc_tab[0][i] >> 8);
    __syncthreads();
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= n_blocks) return;
    const InfBlock blk = blocks[b];
    uint8_t* const out = data + blk.out_off;
    int rc = blk.out_len == 0 ? 0
                              : strk_inf::inflate_block(comp + blk.in_off, blk.in_len, out, blk.out_len, &tabs[threadIdx.x],
                                                        lens_scratch + (size_t)b * strk_inf::kLensBytes);
    if (rc == 0) {
        uint32_t c = 0xffffffffu;
        int i = 0;
        auto step4 = [&](uint32_t w) {              // slice-by-2, two steps per word
            c ^= w & 0xffffu;
            c = crc_tab[1][c & 0xffu] ^ crc_tab[0][(c >> 8) & 0xffu] ^ (c >> 16);
            c ^= w >> 16;
            c = crc_tab[1][c & 0xffu] ^ crc_tab[0][(c >> 8) & 0xffu] ^ (c >> 16);
        };
        // the lane reads its own block back: 128 bytes per trip to memory (sixteen loads in flight), not four — a trip costs
        // more than a microsecond whatever it carries, and a block would need sixteen thousand of them
        for (; i + 128 <= blk.out_len; i += 128) {
            uint64_t w[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) __builtin_memcpy(&w[k], out + i + 8 * k, 8);
#pragma unroll
            for (int k = 0; k < 16; ++k) { step4((uint32_t)w[k]); step4((uint32_t)(w[k] >> 32)); }
        }
        for (; i + 4 <= blk.out_len; i += 4) {
            uint32_t w;
            __builtin_memcpy(&w, out + i, 4);
            step4(w);
        }
        for (; i < blk.out_len; ++i) c = crc_tab[0][(c ^ out[i]) & 0xffu] ^ (c >> 8);
        if ((c ^ 0xffffffffu) != blk.crc) rc = strk_inf::kErrCrc;
    }
    // (block index above the error: the smallest word is the first bad block of the stretch together with its own error)
    if (rc) atomicMin(status, ((unsigned long long)b << 32) | (unsigned long long)rc);
}

// Record scan.  Records follow one another without markers, so a chain has to be walked; the .bai linear index gives the
// offset of a record start every 16 kb of the reference (thousands of entry points), and lane s walks the chain from entry
// point s up to entry point s + 1: once to count its records (first == NULL: counts[s]), then — the host has summed the
// counts — to write them where they belong, first[s] onwards: the arrays come out in file order.
__global__ void __launch_bounds__(256) k_dbam_scan(const uint8_t* data, int64_t n_data, const int64_t* starts, int n_starts, int64_t cap,
                                                   const int64_t* first, int32_t* counts, int64_t* rec_off,
                                                   int32_t* fields /* [8][cap] */, int32_t* status) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_starts) return;
    int64_t off = starts[s];
    const int64_t lim = s + 1 < n_starts ? starts[s + 1] : n_data;
    int64_t k = first ? first[s] : 0;
    int32_t n = 0;
    while (off < lim) {
        // a record that runs past the end of the stretch: the stretch ends at a BGZF block boundary, records do not care about
        // those (the host decides whether that is the end of a span or a truncated file)
        if (off + 4 > n_data) { atomicMax(&status[1], 1); break; }
        const int32_t block = strk_fe::rd_i32(data + off);
        if (block >= 32 && off + 4 + block > n_data) { atomicMax(&status[1], 1); break; }
        strk_fe::Rec r;
        int64_t next = 0;
        if (!strk_fe::parse_rec(data, n_data, off, &r, &next)) { atomicMax(&status[0], 1); return; }
        if (first && k < cap) {
            int64_t ref_len;
            int32_t cl, cr;
            strk_fe::cigar_span(r.cigar, r.n_cigar, &ref_len, &cl, &cr);
            rec_off[k] = off;
            fields[0 * cap + k] = r.tid; fields[1 * cap + k] = r.pos; fields[2 * cap + k] = (int32_t)(r.pos + ref_len);
            fields[3 * cap + k] = r.flag; fields[4 * cap + k] = r.l_seq; fields[5 * cap + k] = cl; fields[6 * cap + k] = cr;
            fields[7 * cap + k] = r.l_name;
        }
        ++k; ++n;
        off = next;
    }
    // a walk that does not END on the next entry point followed an index entry that is not a record start (a stale or foreign
    // .bai): the records of two stretches would be counted twice or cut — an error, not a result
    if (s + 1 < n_starts && off != lim && off < n_data) atomicMax(&status[0], 1);
    if (!first) counts[s] = n;
}

// Read extraction, pass 1: where each item's flank | tract | flank lies in its read (strk_extract_reads, same rules), the
// length of its name.  Pass 2 (after the host has summed the lengths): bases (4 bit -> ASCII, low-quality bases -> 'X').
// alt_*: optional substitute CIGARs (realigned reads), as in strk_extract_reads.
__global__ void __launch_bounds__(256) k_dbam_extract1(const uint8_t* data, int64_t n_data, int n_items, const int64_t* rec_off,
                                                       const int64_t* coords, strk_fe::AltCigars alt, int flank_size, int min_avg_phred,
                                                       int32_t* status, int32_t* nfl, int32_t* ntr, int32_t* nfr, int64_t* cut_a,
                                                       int32_t* name_len, int32_t* bad) {
    const int it = blockIdx.x * blockDim.x + threadIdx.x;
    if (it >= n_items) return;
    status[it] = 1; nfl[it] = 0; ntr[it] = 0; nfr[it] = 0; cut_a[it] = 0; name_len[it] = 0;
    strk_fe::Rec r;
    int64_t next = 0;
    if (!strk_fe::parse_rec(data, n_data, rec_off[it], &r, &next)) { atomicMax(bad, INT32_MAX - it); return; }
    name_len[it] = r.l_name > 0 ? r.l_name - 1 : 0;
    int64_t q[4];
    const uint8_t* cig;
    int32_t n_cig;
    int64_t start;
    strk_fe::item_alignment(r, it, alt, &cig, &n_cig, &start);
    if (!strk_fe::read_coords_linear(cig, n_cig, start, coords[4 * (size_t)it], coords[4 * (size_t)it + 1],
                                     coords[4 * (size_t)it + 2], coords[4 * (size_t)it + 3], q))
        return;
    const int64_t b = q[1], c = q[2];
    const int64_t a = q[0] > b - flank_size ? q[0] : b - flank_size, d = q[3] < c + flank_size ? q[3] : c + flank_size;
    if (a < 0 || d > r.l_seq || a > b || b > c || c > d) return;   // coordinates outside the read: incomplete
    const bool has_qual = !(r.l_seq > 0 && r.qual[0] == 0xFF);
    if (has_qual && c > b) {   // LowMeanBaseQual on the tract bases (call_locus.py:1099-1115)
        int64_t sum = 0;
        for (int64_t i = b; i < c; ++i) sum += r.qual[i];
        if ((double)sum / (double)(c - b) < (double)min_avg_phred) { status[it] = 2; return; }
    }
    status[it] = 0;
    nfl[it] = (int32_t)(b - a); ntr[it] = (int32_t)(c - b); nfr[it] = (int32_t)(d - c);
    cut_a[it] = a;
}

// eight lanes per item: lane l writes bases l, l + 8, ...
__global__ void __launch_bounds__(256) k_dbam_extract2(const uint8_t* data, int64_t n_data, int n_items, const int64_t* rec_off,
                                                       const int32_t* status, const int32_t* nfl, const int32_t* ntr, const int32_t* nfr,
                                                       const int64_t* cut_a, const int64_t* seq_off, int wildcard_threshold, uint8_t* seqs) {
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    const int it = gid >> 3, l = gid & 7;
    if (it >= n_items || status[it] != 0) return;
    strk_fe::Rec r;
    int64_t next = 0;
    if (!strk_fe::parse_rec(data, n_data, rec_off[it], &r, &next)) return;
    const bool has_qual = !(r.l_seq > 0 && r.qual[0] == 0xFF);
    const int64_t a = cut_a[it];
    const int n = nfl[it] + ntr[it] + nfr[it];
    uint8_t* o = seqs + seq_off[it];
    for (int k = l; k < n; k += 8) {
        const int64_t i = a + k;
        const uint8_t byte = r.seq[i >> 1];
        const int code = (i & 1) ? (byte & 15) : (byte >> 4);
        char ch = "=ACMGRSVTWYHKDBN"[code];
        if (has_qual && (int)r.qual[i] <= wildcard_threshold) ch = 'X';
        o[k] = (uint8_t)ch;
    }
}

__global__ void __launch_bounds__(256) k_dbam_names(const uint8_t* data, int n, const int64_t* rec_off, const int64_t* out_off, uint8_t* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t* name = data + rec_off[i] + 4 + 32;
    const int64_t len = out_off[i + 1] - out_off[i];
    for (int64_t k = 0; k < len; ++k) out[out_off[i] + k] = name[k];
}

}  // namespace

// Device buffers of gigabytes are not given back when a reader is closed: the next reader of the process takes them over.
// hipMalloc of a 7 GB buffer right after the hipFree of another one took 0.5-0.7 s in one run out of three (profiles/
// r02_k_open_stages.txt), more than reading, uploading and inflating the file together.  At most two per device (the
// decompressed stream and the compressed bytes); strk_dbam_release_cache() frees them.
namespace {
struct ParkedBuf { int device; DevBuf buf; };
std::mutex g_park_mu;
// (never destroyed: what is parked when the process ends is left to the driver — no HIP call after main() has returned)
std::vector<ParkedBuf>& g_parked = *new std::vector<ParkedBuf>();
std::vector<std::pair<int, PinnedBuf>>& g_parked_rings = *new std::vector<std::pair<int, PinnedBuf>>();   // the pinned rings of closed readers (one per device is kept)

void dbam_park(int device, DevBuf& b) {
    if (!b.p || b.cap < ((size_t)64 << 20)) { b.release(); return; }
    std::lock_guard<std::mutex> lk(g_park_mu);
    int n_dev = 0;
    size_t smallest = (size_t)-1;
    for (size_t i = 0; i < g_parked.size(); ++i)
        if (g_parked[i].device == device) { ++n_dev; if (smallest == (size_t)-1 || g_parked[i].buf.cap < g_parked[smallest].buf.cap) smallest = i; }
    if (n_dev >= 2) {
        if (g_parked[smallest].buf.cap >= b.cap) { b.release(); return; }
        g_parked[smallest].buf.release();
        g_parked.erase(g_parked.begin() + (long)smallest);
    }
    g_parked.push_back(ParkedBuf{device, std::move(b)});
}

// b can hold `bytes` afterwards: as it is, through a parked buffer (the smallest that fits), or through hipMalloc
int dbam_big_ensure(int device, DevBuf& b, size_t bytes) {
    if (bytes <= b.cap) return 0;
    {
        std::lock_guard<std::mutex> lk(g_park_mu);
        size_t best = (size_t)-1;
        for (size_t i = 0; i < g_parked.size(); ++i)
            if (g_parked[i].device == device && g_parked[i].buf.cap >= bytes && (best == (size_t)-1 || g_parked[i].buf.cap < g_parked[best].buf.cap)) best = i;
        if (best != (size_t)-1) {
            b = std::move(g_parked[best].buf);
            g_parked.erase(g_parked.begin() + (long)best);
            return 0;
        }
    }
    return b.ensure(bytes, false);   // exactly: a quarter of head-room on a 100 GB buffer is 25 GB
}
}  // namespace

struct strk_dbam {
    int device = 0;
    DevBuf comp, blocks, data, lens, status;
    // w_a: the staging (strk_host.h) of a call on items: extraction, names, useful SNVs, methylation, selection; the scan's starts
    DevBuf w_a, w_b, w_c, w_d, w_e, w_f, seqs;   // scan / selection work buffers, the extracted bases (until the next extraction)
    // strk_dbam_phase_cells (strk_phase_inputs.inc): the cells of its last call (base | quality) and its staging, of which the
    // cells' offsets per item (at pc_cell_off) and the candidate offsets (at pc_cand_off) serve strk_dbam_useful_snvs: no other
    // entry stages into these two.  And what strk_dbam_useful_snvs checks its input against.
    DevBuf pc_cells, pc_in;
    PinnedBuf stage;   // the host image of the call in progress (Staging)
    size_t pc_cell_off = 0, pc_cand_off = 0;
    std::vector<int32_t> pc_item_locus, pc_cand_off_h;
    std::vector<int64_t> pc_cell_off_h;
    bool pc_valid = false;
    DevBuf sd_masks;   // strk_dbam_discover_snvs (strk_snv_discover.inc): the candidate masks of its tiles, 512 bytes each
    DevBuf ln_tiles, ln_starts, ln_query;   // the lines of a text (strk_lines.inc): per tile, the line starts; a reader's status words and contig name
    DevBuf vc_lines, vc_out;   // strk_dbam_vcf_snvs (strk_vcf.inc): per line, per kept line
    DevBuf gf_lines, gf_feat, gf_join, gf_pairs, gf_out, gf_text;   // strk_dbam_gff_overlaps (strk_gff.inc): per line, feature, locus, pair; what is downloaded
    int64_t n_data = 0;    // bytes of `data` that are filled
    int64_t coff0 = 0;     // compressed offset of the inflated stretch
    PinnedBuf ring_mem;                     // strk_dbam_inflate_file: pinned pieces, their stream and events
    Stream ring_stream;
    Event ring_ev[6];
    bool to_eof = true;    // the stretch runs to the end of its file / buffer (a record cut off at its end is then an error)
    std::vector<int64_t> blk_coff, blk_out;   // per inflated block: its compressed offset and where its bytes start in `data`
    std::vector<int32_t> blk_len;
    Event ev0, ev1;
    double kernel_ms = 0.0;   // HIP-event time of every kernel this object has launched
    double file_ms[3] = {0.0, 0.0, 0.0};   // last strk_dbam_inflate_file: buffers, read + upload, inflation (wall clock)
    void tic() { if (ev0) (void)hipEventRecord(ev0, 0); }
    void toc() {
        float ms = 0.f;
        if (ev0 && ev1 && hipEventRecord(ev1, 0) == hipSuccess && hipEventSynchronize(ev1) == hipSuccess &&
            hipEventElapsedTime(&ms, ev0, ev1) == hipSuccess)
            kernel_ms += ms;
    }
};

// One BGZF block header at compressed offset `off`: `get(o, n, tmp)` hands out n contiguous bytes of the file at offset o
// (<= 65536 + 18 of them).  Fills the descriptor (offsets relative to `coff`, out_off left to the caller); *next = the offset
// of the following block.
template <class Get>
static int dbam_block_at(Get&& get, int64_t off, int64_t n_comp, int64_t coff, InfBlock* b, int64_t* next_out) {
    uint8_t tmp[65536 + 32];
    if (off + 18 > n_comp) return fail(STRK_E_INVALID, "truncated BGZF block header at byte %lld", (long long)off);
    const uint8_t* p = get(off, 12, tmp);
    if (p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || !(p[3] & 4)) return fail(STRK_E_INVALID, "not a BGZF block at byte %lld", (long long)off);
    const int xlen = strk_fe::rd_u16(p + 10);
    if (off + 12 + xlen > n_comp) return fail(STRK_E_INVALID, "truncated BGZF block header at byte %lld", (long long)off);
    p = get(off, 12 + xlen, tmp);
    int bsize = -1;
    for (int x = 12; x + 4 <= 12 + xlen;) {
        const int slen = strk_fe::rd_u16(p + x + 2);
        if (p[x] == 'B' && p[x + 1] == 'C' && slen == 2 && x + 6 <= 12 + xlen) bsize = strk_fe::rd_u16(p + x + 4);
        x += 4 + slen;
    }
    const int64_t next = off + bsize + 1;
    if (bsize < 0 || next > n_comp || next - 8 < off + 12 + xlen) return fail(STRK_E_INVALID, "truncated BGZF block at byte %lld", (long long)off);
    const uint8_t* t = get(next - 8, 8, tmp);
    b->in_off = off + 12 + xlen - coff;
    b->in_len = (int32_t)(next - 8 - (off + 12 + xlen));
    b->crc = strk_fe::rd_u32(t);
    b->out_len = (int32_t)strk_fe::rd_u32(t + 4);
    b->out_off = 0;
    b->pad = 0;
    if (b->out_len < 0 || b->out_len > 65536) return fail(STRK_E_INVALID, "bad BGZF block at byte %lld", (long long)off);
    *next_out = next;
    return 0;
}

// The compressed bytes [coff, coff + n_in) are in d->comp (or on their way there on `stream`): inflates `blocks`.
static int64_t dbam_run_inflate(strk_dbam* d, const std::vector<InfBlock>& blocks, int64_t n_in, int64_t total, int64_t coff, hipStream_t stream) {
    int rc;
    if ((rc = d->blocks.ensure(blocks.size() * sizeof(InfBlock))) || (rc = dbam_big_ensure(d->device, d->data, (size_t)total + 16)) ||
        (rc = d->lens.ensure(blocks.size() * (size_t)strk_inf::kLensBytes)) || (rc = d->status.ensure(8)))
        return rc;
    const uint64_t st0 = UINT64_MAX;   // no bad block
    HIP_TRY(hipStreamSynchronize(stream));
    HIP_TRY(hipMemset(d->comp.as<uint8_t>() + n_in, 0, 16));
    HIP_TRY(hipMemcpy(d->blocks.p, blocks.data(), blocks.size() * sizeof(InfBlock), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d->status.p, &st0, 8, hipMemcpyHostToDevice));
    const int nb = (int)blocks.size();
    d->tic();
    hipLaunchKernelGGL(k_bgzf_inflate, dim3((nb + 63) / 64), dim3(64), 0, 0, d->comp.as<uint8_t>(), d->blocks.as<InfBlock>(), nb,
                       d->data.as<uint8_t>(), d->lens.as<uint8_t>(), d->status.as<unsigned long long>());
    HIP_TRY(hipGetLastError());
    d->toc();
    uint64_t st = 0;
    HIP_TRY(hipMemcpy(&st, d->status.p, 8, hipMemcpyDeviceToHost));
    if (st != st0)
        return fail(STRK_E_INVALID, "corrupt BGZF block %d of the stretch at byte %lld (%s)", (int)(st >> 32), (long long)coff,
                    (int)(st & 0xffffffffu) == strk_inf::kErrCrc ? "CRC mismatch" : "inflate failed");
    d->n_data = total;
    return total;
}

extern "C" {

int strk_dbam_open(int device, strk_dbam** out) {
    if (!out) return fail(STRK_E_INVALID, "out is NULL");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return fail(STRK_E_DEVICE, "no such HIP device %d", device);
    HIP_TRY(hipSetDevice(device));
    strk_dbam* d = new strk_dbam();
    d->device = device;
    (void)hipEventCreate(&d->ev0.h);
    (void)hipEventCreate(&d->ev1.h);
    *out = d;
    return 0;
}

void strk_dbam_close(strk_dbam* d) {
    if (!d) return;
    (void)hipSetDevice(d->device);
    dbam_park(d->device, d->data);
    dbam_park(d->device, d->comp);
    if (d->ring_stream) (void)hipStreamSynchronize(d->ring_stream);
    if (d->ring_mem.p) {   // one pinned ring per device is kept for the next reader
        std::lock_guard<std::mutex> lk(g_park_mu);
        bool have = false;
        for (auto& r : g_parked_rings) have = have || r.first == d->device;
        if (!have) g_parked_rings.emplace_back(d->device, std::move(d->ring_mem));
    }
    delete d;
}

// Inflates the consecutive BGZF blocks of `comp` (host memory: the compressed file or a stretch of it) that start at byte
// `coff`, as many as decompress into at most `max_out` bytes, into the object's device buffer (replacing its content).
// Returns the decompressed bytes (>= 0) or a negative error; *next_coff = offset of the first block not taken.
int64_t strk_dbam_inflate(strk_dbam* d, const uint8_t* comp, int64_t n_comp, int64_t coff, int64_t max_out, int64_t* next_coff) {
    if (!d || !comp || !next_coff || n_comp < 0 || coff < 0 || coff > n_comp || max_out < 0) return fail(STRK_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(d->device));
    std::vector<InfBlock> blocks;
    d->blk_coff.clear(); d->blk_out.clear(); d->blk_len.clear();
    d->coff0 = coff;
    d->n_data = 0;
    int64_t off = coff, total = 0;
    auto get = [&](int64_t o, int, uint8_t*) { return comp + o; };
    while (off < n_comp) {
        InfBlock b;
        int64_t next = 0;
        const int rc = dbam_block_at(get, off, n_comp, coff, &b, &next);
        if (rc) return rc;
        if (total + b.out_len > max_out) break;
        b.out_off = total;
        d->blk_coff.push_back(off); d->blk_out.push_back(total); d->blk_len.push_back(b.out_len);
        total += b.out_len;
        blocks.push_back(b);
        off = next;
    }
    *next_coff = off;
    d->to_eof = off >= n_comp;
    if (blocks.empty()) return 0;
    const int64_t n_in = off - coff;
    const int rc = dbam_big_ensure(d->device, d->comp, (size_t)n_in + 16);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(d->comp.p, comp + coff, (size_t)n_in, hipMemcpyHostToDevice));
    return dbam_run_inflate(d, blocks, n_in, total, coff, 0);
}

// The same for a whole file, read here: `threads` readers pread 8 MB pieces of it into a ring of pinned buffers, each piece
// goes to the device as soon as it is in (asynchronous copies on one stream) while this thread walks the block headers of the
// pieces that are in, and the blocks are inflated by one launch when the last piece has landed.  Neither a second host copy
// of the file nor a pass of the runtime over pageable memory: the file moves at what the page cache and PCIe give.
// Returns the decompressed bytes (>= 0) or a negative error; *n_comp = size of the file.
// strk_dbam_inflate_file_range: the same for the BGZF blocks of the file's bytes [coff_lo, coff_hi) (both block boundaries;
// coff_hi < 0 or past the end: up to the end of the file) — a file that does not fit in device memory goes through it span by
// span.
static int64_t dbam_inflate_file_impl(strk_dbam* d, const char* path, int64_t lo, int64_t hi, int threads, int64_t* n_comp_out) {
    if (!d || !path || lo < 0) return fail(STRK_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(d->device));
    const int fd = ::open(path, O_RDONLY);
    if (fd < 0) return fail(STRK_E_INVALID, "cannot open %s", path);
    struct stat sb;
    if (::fstat(fd, &sb) != 0 || sb.st_size < 0) { ::close(fd); return fail(STRK_E_INVALID, "cannot stat %s", path); }
    if (n_comp_out) *n_comp_out = (int64_t)sb.st_size;
    if (hi < 0 || hi > (int64_t)sb.st_size) hi = (int64_t)sb.st_size;
    d->to_eof = hi == (int64_t)sb.st_size;
    if (lo > hi) { ::close(fd); return fail(STRK_E_INVALID, "range starts past the end of %s", path); }
    const int64_t n = hi - lo;                 // every offset below is relative to `lo`
    d->blk_coff.clear(); d->blk_out.clear(); d->blk_len.clear();
    d->coff0 = lo;
    d->n_data = 0;
    if (n == 0) { ::close(fd); return 0; }
    const auto clk0 = std::chrono::steady_clock::now();
    auto since = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - clk0).count(); };
    constexpr int64_t kPiece = 8 << 20;
    constexpr int kRing = 6;
    const int64_t n_pieces = (n + kPiece - 1) / kPiece;
    const int ring = (int)std::min<int64_t>(kRing, n_pieces);
    threads = std::max(1, std::min(threads > 0 ? threads : 6, (int)std::min<int64_t>(n_pieces, 16)));
    int rc = dbam_big_ensure(d->device, d->comp, (size_t)n + 16);
    if (rc) { ::close(fd); return rc; }
    // the ring of pinned pieces, its stream and events belong to the object: a file walked span by span allocates them once
    hipError_t he = hipSuccess;
    if (!d->ring_mem.p) {
        std::lock_guard<std::mutex> lk(g_park_mu);
        for (size_t i = 0; i < g_parked_rings.size(); ++i)
            if (g_parked_rings[i].first == d->device) {
                d->ring_mem = std::move(g_parked_rings[i].second);
                g_parked_rings.erase(g_parked_rings.begin() + (long)i);
                break;
            }
    }
    if (!d->ring_mem.p) he = d->ring_mem.alloc((size_t)kRing * kPiece);
    if (he == hipSuccess && !d->ring_stream) he = hipStreamCreateWithFlags(&d->ring_stream.h, hipStreamNonBlocking);
    for (int i = 0; i < kRing && he == hipSuccess; ++i)
        if (!d->ring_ev[i]) he = hipEventCreateWithFlags(&d->ring_ev[i].h, hipEventDisableTiming);
    uint8_t* const pinned = d->ring_mem.as<uint8_t>();
    const hipStream_t stream = d->ring_stream;
    Event* const ev = d->ring_ev;
    std::mutex mu;
    std::condition_variable cv;
    std::vector<char> loaded((size_t)n_pieces, 0);
    int64_t freed = 0;          // pieces whose ring slot may be overwritten (everything below this index is done with)
    std::atomic<int64_t> next_piece{0};
    bool stop = false, io_error = false;
    auto reader = [&]() {
        for (;;) {
            const int64_t c = next_piece.fetch_add(1);
            if (c >= n_pieces) return;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return stop || freed > c - ring; });
                if (stop) return;
            }
            uint8_t* dst = pinned + (size_t)(c % ring) * kPiece;
            const int64_t want = std::min(kPiece, n - c * kPiece);
            int64_t got = 0;
            while (got < want) {
                const ssize_t k = ::pread(fd, dst + got, (size_t)(want - got), (off_t)(lo + c * kPiece + got));
                if (k <= 0) break;
                got += k;
            }
            std::lock_guard<std::mutex> lk(mu);
            if (got < want) io_error = true;
            loaded[(size_t)c] = 1;
            cv.notify_all();
        }
    };
    const double t_alloc = since();
    std::vector<std::thread> pool;
    if (he == hipSuccess)
        for (int i = 0; i < threads; ++i) pool.emplace_back(reader);
    std::vector<InfBlock> blocks;
    int64_t copied = 0, walked = 0, off = 0, total = 0;
    // n contiguous bytes of the file at offset o, out of the ring (a block lies in at most two consecutive pieces)
    auto get = [&](int64_t o, int len, uint8_t* tmp) -> const uint8_t* {
        const int64_t c = o / kPiece, in = o % kPiece;
        const uint8_t* a = pinned + (size_t)(c % ring) * kPiece + in;
        if (in + len <= kPiece) return a;
        const int first = (int)(kPiece - in);
        __builtin_memcpy(tmp, a, (size_t)first);
        __builtin_memcpy(tmp + first, pinned + (size_t)((c + 1) % ring) * kPiece, (size_t)(len - first));
        return tmp;
    };
    rc = 0;
    while (he == hipSuccess && rc == 0 && walked < n_pieces) {
        bool progress = false;
        {   // pieces that have come in, in order -> device
            std::unique_lock<std::mutex> lk(mu);
            if (io_error) { rc = fail(STRK_E_INVALID, "read error on %s", path); break; }
            while (copied < n_pieces && loaded[(size_t)copied]) {
                lk.unlock();
                const int64_t len = std::min(kPiece, n - copied * kPiece);
                he = hipMemcpyAsync(d->comp.as<uint8_t>() + copied * kPiece, pinned + (size_t)(copied % ring) * kPiece, (size_t)len,
                                    hipMemcpyHostToDevice, stream);
                if (he == hipSuccess) he = hipEventRecord(ev[(size_t)(copied % ring)], stream);
                ++copied;
                progress = true;
                lk.lock();
                if (he != hipSuccess) break;
            }
        }
        if (he != hipSuccess) break;
        // the blocks that start in piece `walked` (they end in the next one at the latest)
        if (walked < copied && (walked + 1 < copied || copied == n_pieces)) {
            const int64_t lim = std::min(n, (walked + 1) * kPiece);
            while (off < lim && rc == 0) {
                InfBlock b;
                int64_t next = 0;
                rc = dbam_block_at(get, off, n, 0, &b, &next);
                if (rc) break;
                b.out_off = total;
                d->blk_coff.push_back(lo + off); d->blk_out.push_back(total); d->blk_len.push_back(b.out_len);
                total += b.out_len;
                blocks.push_back(b);
                off = next;
            }
            ++walked;
            progress = true;
        }
        // slots of pieces that are walked and on the device go back to the readers
        while (rc == 0 && freed < walked && freed < copied) {
            const hipError_t q = progress ? hipEventQuery(ev[(size_t)(freed % ring)]) : hipEventSynchronize(ev[(size_t)(freed % ring)]);
            if (q == hipErrorNotReady) break;
            if (q != hipSuccess) { he = q; break; }
            std::lock_guard<std::mutex> lk(mu);
            ++freed;
            cv.notify_all();
            progress = true;
        }
        if (!progress) {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return io_error || (copied < n_pieces && loaded[(size_t)copied]); });
        }
    }
    {
        std::lock_guard<std::mutex> lk(mu);
        stop = true;
        cv.notify_all();
    }
    for (auto& t : pool) t.join();
    ::close(fd);
    const double t_read = since();
    int64_t out = rc;
    if (he != hipSuccess) out = fail(STRK_E_DEVICE, "HIP error while uploading %s: %s", path, hipGetErrorString(he));
    else if (rc == 0) out = blocks.empty() ? 0 : dbam_run_inflate(d, blocks, n, total, lo, stream);
    if (stream) (void)hipStreamSynchronize(stream);
    if (out < 0) { d->blk_coff.clear(); d->blk_out.clear(); d->blk_len.clear(); }
    d->file_ms[0] = t_alloc; d->file_ms[1] = t_read - t_alloc; d->file_ms[2] = since() - t_read;
    return out;
}

// Copies bytes [off, off + n) of the decompressed stream to the host (headers, single records for realignment, tests).
int strk_dbam_download(strk_dbam* d, int64_t off, int64_t n, uint8_t* out) {
    if (!d || !out || off < 0 || n < 0 || off + n > d->n_data) return fail(STRK_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(d->device));
    if (n) HIP_TRY(hipMemcpy(out, d->data.as<uint8_t>() + off, (size_t)n, hipMemcpyDeviceToHost));
    return 0;
}

// The first n bytes of the bases the last strk_dbam_extract produced -> host (tests).
int strk_dbam_download_seqs(strk_dbam* d, int64_t n, uint8_t* out) {
    if (!d || !out || n < 0 || (size_t)n > d->seqs.cap) return fail(STRK_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(d->device));
    if (n) HIP_TRY(hipMemcpy(out, d->seqs.p, (size_t)n, hipMemcpyDeviceToHost));
    return 0;
}

// Frees the device buffers that closed readers have left for the next one (see dbam_park).
void strk_dbam_release_cache(void) {
    std::lock_guard<std::mutex> lk(g_park_mu);
    for (auto& pb : g_parked) {
        (void)hipSetDevice(pb.device);
        pb.buf.release();
    }
    g_parked.clear();
    for (auto& r : g_parked_rings) {
        (void)hipSetDevice(r.first);
        r.second.release();
    }
    g_parked_rings.clear();
}

// HIP-event time (ms) of all kernels the object has launched so far (inflation, scan, extraction).
double strk_dbam_kernel_ms(strk_dbam* d) { return d ? d->kernel_ms : 0.0; }

int64_t strk_dbam_inflate_file(strk_dbam* d, const char* path, int threads, int64_t* n_comp_out) {
    return dbam_inflate_file_impl(d, path, 0, -1, threads, n_comp_out);
}
int64_t strk_dbam_inflate_file_range(strk_dbam* d, const char* path, int64_t coff_lo, int64_t coff_hi, int threads, int64_t* n_comp_out) {
    return dbam_inflate_file_impl(d, path, coff_lo, coff_hi, threads, n_comp_out);
}

// Wall-clock stages (ms) of the last strk_dbam_inflate_file: buffers (device + pinned ring), read + upload, inflation.
void strk_dbam_file_ms(strk_dbam* d, double* out3) {
    for (int i = 0; i < 3; ++i) out3[i] = d ? d->file_ms[i] : 0.0;
}

// The device address of the decompressed stream (valid until the next strk_dbam_inflate / strk_dbam_close).
void* strk_dbam_data(strk_dbam* d, int64_t* n_bytes) {
    if (n_bytes) *n_bytes = d ? d->n_data : 0;
    return d ? d->data.p : nullptr;
}

// BAM virtual offsets (compressed offset of a BGZF block << 16 | offset inside its decompressed bytes) -> offsets in the
// decompressed stream of the inflated stretch; -1 for an offset that does not point into it.
int strk_dbam_voffsets(strk_dbam* d, const uint64_t* voff, int64_t n, int64_t* out) {
    if (!d || n < 0 || (n > 0 && (!voff || !out))) return fail(STRK_E_INVALID, "bad argument");
    for (int64_t i = 0; i < n; ++i) {
        const int64_t coff = (int64_t)(voff[i] >> 16), u = (int64_t)(voff[i] & 0xFFFF);
        const auto itb = std::lower_bound(d->blk_coff.begin(), d->blk_coff.end(), coff);
        out[i] = -1;
        if (itb != d->blk_coff.end() && *itb == coff) {
            const size_t k = (size_t)(itb - d->blk_coff.begin());
            // (an offset equal to the block's length is the start of the next block: htslib writes such offsets)
            if (u <= d->blk_len[k] && d->blk_out[k] + u <= d->n_data) out[i] = d->blk_out[k] + u;
        }
    }
    return 0;
}

// Record scan on the device: `starts` = ascending, distinct offsets of record starts (the first record and what the index
// points at); every record from starts[0] to the end of the stretch is reported once.  Returns the number of records; the
// host arrays (capacity `cap`) are filled, in file order, when that number fits (two passes: count, then write in place).
int64_t strk_dbam_scan(strk_dbam* d, const int64_t* starts, int64_t n_starts, int64_t cap, int64_t* rec_off, int32_t* tid,
                       int32_t* pos, int32_t* end, int32_t* flag, int32_t* l_seq, int32_t* clip_l, int32_t* clip_r, int32_t* l_name) {
    if (!d || n_starts < 0 || cap < 0 || (n_starts > 0 && !starts)) return fail(STRK_E_INVALID, "bad argument");
    if (cap > 0 && (!rec_off || !tid || !pos || !end || !flag || !l_seq || !clip_l || !clip_r || !l_name)) return fail(STRK_E_INVALID, "NULL output array");
    if (n_starts == 0 || d->n_data == 0) return 0;
    for (int64_t i = 0; i < n_starts; ++i)
        if (starts[i] < 0 || starts[i] > d->n_data || (i && starts[i] <= starts[i - 1])) return fail(STRK_E_INVALID, "starts must be ascending offsets into the stream");
    HIP_TRY(hipSetDevice(d->device));
    int rc;
    if ((rc = d->w_a.ensure((size_t)n_starts * 8)) || (rc = d->w_d.ensure((size_t)n_starts * 4)) || (rc = d->status.ensure(8))) return rc;
    HIP_TRY(hipMemcpy(d->w_a.p, starts, (size_t)n_starts * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(d->status.p, 0, 8));
    const dim3 grid((unsigned)((n_starts + 255) / 256));
    // pass 1: records per entry point
    d->tic();
    hipLaunchKernelGGL(k_dbam_scan, grid, dim3(256), 0, 0, d->data.as<uint8_t>(), d->n_data, d->w_a.as<int64_t>(), (int)n_starts, (int64_t)0,
                       (const int64_t*)nullptr, d->w_d.as<int32_t>(), (int64_t*)nullptr, (int32_t*)nullptr, d->status.as<int32_t>());
    HIP_TRY(hipGetLastError());
    d->toc();
    int32_t st[2];
    HIP_TRY(hipMemcpy(st, d->status.p, 8, hipMemcpyDeviceToHost));
    if (st[0]) return fail(STRK_E_INVALID, "malformed BAM record in the stretch");
    if (st[1] && d->to_eof) return fail(STRK_E_INVALID, "malformed BAM record in the stretch (the last record is cut off: truncated file)");
    std::vector<int32_t> counts((size_t)n_starts);
    HIP_TRY(hipMemcpy(counts.data(), d->w_d.p, (size_t)n_starts * 4, hipMemcpyDeviceToHost));
    std::vector<int64_t> first((size_t)n_starts);
    int64_t n = 0;
    for (int64_t i = 0; i < n_starts; ++i) { first[(size_t)i] = n; n += counts[(size_t)i]; }
    if (n > cap || n == 0) return n;
    // pass 2: every record to its place; the fields of `n` records, back to back
    if ((rc = d->w_b.ensure((size_t)n * 8)) || (rc = d->w_c.ensure((size_t)n * 8 * 4)) || (rc = d->w_e.ensure((size_t)n_starts * 8))) return rc;
    HIP_TRY(hipMemcpy(d->w_e.p, first.data(), (size_t)n_starts * 8, hipMemcpyHostToDevice));
    d->tic();
    hipLaunchKernelGGL(k_dbam_scan, grid, dim3(256), 0, 0, d->data.as<uint8_t>(), d->n_data, d->w_a.as<int64_t>(), (int)n_starts, n,
                       d->w_e.as<int64_t>(), (int32_t*)nullptr, d->w_b.as<int64_t>(), d->w_c.as<int32_t>(), d->status.as<int32_t>());
    HIP_TRY(hipGetLastError());
    d->toc();
    HIP_TRY(hipMemcpy(rec_off, d->w_b.p, (size_t)n * 8, hipMemcpyDeviceToHost));
    int32_t* outs[8] = {tid, pos, end, flag, l_seq, clip_l, clip_r, l_name};
    for (int j = 0; j < 8; ++j) HIP_TRY(hipMemcpy(outs[j], d->w_c.as<int32_t>() + (size_t)j * n, (size_t)n * 4, hipMemcpyDeviceToHost));
    return (int64_t)n;
}

// strk_extract_reads on the device, for records of the inflated stretch: the bases stay in HBM (*d_seqs, owned by the object
// until the next call), status / lengths / seq_off / name lengths come back to the host.  alt_* as in strk_extract_reads
// (host arrays, may be NULL).
int strk_dbam_extract(strk_dbam* d, int32_t n_items, const int64_t* rec_off, const int64_t* coords, const uint32_t* alt_cigar,
                      const int64_t* alt_cigar_off, const int64_t* alt_start, int32_t flank_size, int32_t min_avg_phred,
                      int32_t wildcard_threshold, int32_t* status, int32_t* nfl, int32_t* ntr, int32_t* nfr, int64_t* seq_off,
                      int32_t* name_len, void** d_seqs) {
    if (!d || n_items < 0 || flank_size < 0 || !d_seqs) return fail(STRK_E_INVALID, "bad argument");
    *d_seqs = nullptr;
    if (n_items == 0) { if (seq_off) seq_off[0] = 0; return 0; }
    if (!rec_off || !coords || !status || !nfl || !ntr || !nfr || !seq_off || !name_len) return fail(STRK_E_INVALID, "NULL argument");
    // before any launch: every offset leaves room for a record's fixed part inside the stream (the kernels' parser checks the rest)
    for (int32_t it = 0; it < n_items; ++it)
        if (rec_off[it] < 0 || rec_off[it] > d->n_data - 36)
            return fail(STRK_E_INVALID, "item %d: record offset %lld outside the stream", it, (long long)rec_off[it]);
    const strk_fe::AltCigars alt{alt_cigar, alt_cigar_off, alt_start};
    strk_groups::Message msg;
    if (strk_fe::check_alt(n_items, alt, &msg)) return fail(STRK_E_INVALID, "%s", msg.text);
    HIP_TRY(hipSetDevice(d->device));
    const size_t n = (size_t)n_items;
    int rc;
    // w_a: rec_off | coords | alt | bad || status nfl ntr nfr name_len || cut_a | seq_off
    Staging st(d->stage);
    const size_t o_rec = st.put(rec_off, n * 8), o_coords = st.put(coords, n * 32);
    const StagedAlt s_alt = stage_alt(st, n, alt);
    const size_t o_bad = st.zero(4), o_out = st.room(n * 4 * 5), o_cut = st.room(n * 8), o_soff = st.room((n + 1) * 8);
    if ((rc = st.upload(d->w_a))) return rc;
    int64_t* const d_rec = d->w_a.at<int64_t>(o_rec);
    int32_t* const d_status = d->w_a.at<int32_t>(o_out);
    int32_t *const d_nfl = d_status + n, *const d_ntr = d_nfl + n, *const d_nfr = d_ntr + n, *const d_nl = d_nfr + n;
    d->tic();
    hipLaunchKernelGGL(k_dbam_extract1, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d->data.as<uint8_t>(), d->n_data, n_items,
                       d_rec, d->w_a.at<int64_t>(o_coords), s_alt.on(d->w_a), flank_size, min_avg_phred, d_status, d_nfl, d_ntr, d_nfr,
                       d->w_a.at<int64_t>(o_cut), d_nl, d->w_a.at<int32_t>(o_bad));
    HIP_TRY(hipGetLastError());
    d->toc();
    if ((rc = st.download(d->w_a, o_bad, o_cut))) return rc;
    const int64_t bad = strk_threads::first_bad_of_word(*st.at<int32_t>(o_bad), INT32_MAX);
    if (bad >= 0) return fail(STRK_E_INVALID, "item %d: malformed BAM record", (int)bad);
    int32_t* const outs[5] = {status, nfl, ntr, nfr, name_len};
    for (int j = 0; j < 5; ++j) memcpy(outs[j], st.at<int32_t>(o_out) + (size_t)j * n, n * 4);
    int64_t w = 0;
    seq_off[0] = 0;
    for (size_t it = 0; it < n; ++it) {
        w += (int64_t)nfl[it] + ntr[it] + nfr[it];
        seq_off[it + 1] = w;
    }
    if ((rc = d->seqs.ensure((size_t)w + 16))) return rc;
    HIP_TRY(hipMemcpy(d->w_a.at<char>(o_soff), seq_off, (n + 1) * 8, hipMemcpyHostToDevice));
    d->tic();
    hipLaunchKernelGGL(k_dbam_extract2, dim3((unsigned)((n * 8 + 255) / 256)), dim3(256), 0, 0, d->data.as<uint8_t>(), d->n_data, n_items,
                       d_rec, d_status, d_nfl, d_ntr, d_nfr, d->w_a.at<int64_t>(o_cut), d->w_a.at<int64_t>(o_soff), wildcard_threshold,
                       d->seqs.as<uint8_t>());
    HIP_TRY(hipGetLastError());
    d->toc();
    *d_seqs = d->seqs.p;
    return 0;
}

// Read names of n records (strk_bam_names' contract, out_off [n + 1] is an INPUT here: the running sum of the name lengths
// strk_dbam_extract reported); fills out[0 .. out_off[n]).
int strk_dbam_names(strk_dbam* d, int64_t n, const int64_t* rec_off, const int64_t* out_off, uint8_t* out) {
    if (!d || n < 0 || n > INT32_MAX || (n > 0 && (!rec_off || !out_off || !out))) return fail(STRK_E_INVALID, "bad argument");
    if (n == 0) return 0;
    // before any launch (k_dbam_names parses nothing): the name slices ascend from 0 and every one lies inside the stream
    if (out_off[0] != 0) return fail(STRK_E_INVALID, "item 0: out_off must ascend from 0");
    for (int64_t i = 0; i < n; ++i) {
        const int64_t len = out_off[i + 1] - out_off[i];
        if (len < 0) return fail(STRK_E_INVALID, "item %lld: out_off must ascend from 0", (long long)i);
        if (rec_off[i] < 0 || rec_off[i] > d->n_data - 36)
            return fail(STRK_E_INVALID, "item %lld: record offset %lld outside the stream", (long long)i, (long long)rec_off[i]);
        if (len > d->n_data - 36 - rec_off[i])
            return fail(STRK_E_INVALID, "item %lld: a name of %lld bytes runs past the stream", (long long)i, (long long)len);
    }
    if (out_off[n] == 0) return 0;
    HIP_TRY(hipSetDevice(d->device));
    // w_a: rec_off | out_off || the names
    Staging st(d->stage);
    const size_t o_rec = st.put(rec_off, (size_t)n * 8), o_off = st.put(out_off, (size_t)(n + 1) * 8), o_out = st.room((size_t)out_off[n] + 16);
    int rc;
    if ((rc = st.upload(d->w_a))) return rc;
    hipLaunchKernelGGL(k_dbam_names, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d->data.as<uint8_t>(), (int)n, d->w_a.at<int64_t>(o_rec),
                       d->w_a.at<int64_t>(o_off), d->w_a.at<uint8_t>(o_out));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, d->w_a.at<char>(o_out), (size_t)out_off[n], hipMemcpyDeviceToHost));   // (straight into the caller's bytes)
    return 0;
}

// Both statements of the CIGAR -> locus boundaries walk on one alignment (test aid): bit 0 of the result = the run-index one
// (strk_frontend.h) found the read spanning, bit 1 = the one-pass one (strk_bamrec.h, what the device runs).
int strk_read_coords_both(const uint32_t* cigar, int32_t n_cigar, int64_t start, const int64_t* coords, int64_t* out_runs, int64_t* out_linear) {
    if (!cigar || n_cigar < 0 || !coords || !out_runs || !out_linear) return fail(STRK_E_INVALID, "bad argument");
    strk_fe::Runs runs;
    runs.build(reinterpret_cast<const uint8_t*>(cigar), n_cigar, start);
    const bool a = strk_fe::read_coords(runs, coords[0], coords[1], coords[2], coords[3], out_runs);
    const bool b = strk_fe::read_coords_linear(reinterpret_cast<const uint8_t*>(cigar), n_cigar, start, coords[0], coords[1], coords[2], coords[3], out_linear);
    return (a ? 1 : 0) | (b ? 2 : 0);
}

// The device inflater's own code on the host, one thread (test aid: tests/test_frontend.py runs it on a CPU-only machine
// against zlib).  Same contract as strk_bgzf_inflate.
int64_t strk_bgzf_inflate_sw(const uint8_t* comp, int64_t n_comp, uint8_t* out, int64_t out_cap) {
    if (!comp || n_comp < 0) return fail(STRK_E_INVALID, "bad argument");
    std::vector<strk_fe::BgzfBlock> blocks;
    int64_t total = 0, bad = 0;
    if (strk_fe::bgzf_index(comp, n_comp, &blocks, &total, &bad))
        return fail(STRK_E_INVALID, "not a BGZF stream (or truncated): bad BGZF block at byte %lld", (long long)bad);
    if (!out) return total;
    if (out_cap < total) return fail(STRK_E_NOMEM, "output buffer too small (%lld < %lld)", (long long)out_cap, (long long)total);
    uint32_t tab[256];
    for (int i = 0; i < 256; ++i) strk_inf::crc_table_entry(tab, i);
    std::vector<uint8_t> in;
    strk_inf::Tables t;
    uint8_t lens[strk_inf::kLensBytes];
    for (const auto& b : blocks) {
        if (b.out_len == 0) continue;
        in.assign(comp + b.in_off, comp + b.in_off + b.in_len);
        in.resize(in.size() + 16, 0);
        const int rc = strk_inf::inflate_block(in.data(), b.in_len, out + b.out_off, b.out_len, &t, lens);
        if (rc) return fail(STRK_E_INVALID, "corrupt BGZF block (inflate error %d)", rc);
        if (strk_inf::crc32_bytes(tab, out + b.out_off, b.out_len) != b.crc) return fail(STRK_E_INVALID, "corrupt BGZF block (CRC)");
    }
    return total;
}

}  // extern "C"
