"""CPU: host logic and the C-ABI surface (no compute calls: there is no GPU in this container)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from helpers import FakeRef, fake_rows, gloo_blocks, oracle_count
from strkit_amd import _build, _lib
from strkit_amd.repeat_count_params import RepeatCountParams, default_read_rc_params, get_reference_rc_params
from strkit_amd.synth import CONFIGS, LocusBatch, make_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_functions():
    src = open(os.path.join(ROOT, "include", "strkit_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(strk_[a-z0-9_]+)\s*\(", src)))


def test_library_builds_loads_and_exports_every_declared_symbol():
    path = _build.build()
    assert os.path.exists(path)
    lib = _lib.load(build=False)
    declared = _header_functions()
    assert declared == sorted(_lib.EXPORTS)
    for name in declared:
        assert getattr(lib, name) is not None
    # the code object inside is gfx950 only
    blob = open(path, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in blob
    for other in (b"gfx90a", b"gfx942", b"sm_80", b"sm_90"):
        assert b"amdhsa--" + other not in blob and other + b"\0" not in blob[:0]
    assert b"gfx950" in lib.strk_version()


def test_host_register_rejects_bad_arguments_before_touching_the_device():
    lib = _lib.load(build=False)
    assert lib.strk_host_register(None, 16) == _lib.STRK_E_INVALID
    assert b"strk_host_register" in lib.strk_last_error()
    buf = (C.c_uint8 * 16)()
    assert lib.strk_host_register(C.cast(buf, C.c_void_p), 0) == _lib.STRK_E_INVALID
    assert lib.strk_host_unregister(None) == _lib.STRK_E_INVALID
    assert lib.strk_host_is_pinned(None, 16) == 0


def test_init_fails_loudly_without_a_gpu_and_errors_are_reported():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by the gpu tests")
    lib = _lib.load(build=False)
    h = C.c_void_p()
    rc = lib.strk_init(0, C.byref(h))
    assert rc != 0 and not h.value
    assert lib.strk_last_error()
    with pytest.raises(_lib.StrkError):
        _lib.Context(0)
    # NULL context / bad arguments are rejected, never dereferenced
    assert lib.strk_count_loci(None, None, None, None, None, None, None, None) == -22
    assert lib.strk_score_table(None, None, None, None, None, 15, 0, None, None) == -22
    from strkit_amd.repeats import get_repeat_count
    with pytest.raises(RuntimeError):  # product path has no CPU fallback
        get_repeat_count(3, "CAGCAGCAG", "ACGT", "TTGA", "CAG", default_read_rc_params())


def test_struct_layouts_match_the_header():
    assert C.sizeof(_lib.StrkParams) == 40
    assert C.sizeof(_lib.StrkStats) == 168
    assert C.sizeof(_lib.StrkBatch) == 8 + 9 * 8


def test_repeat_count_params_mirror_the_reference():
    p = default_read_rc_params()
    assert (p.method, p.max_iters, p.initial_local_search_range, p.initial_step_size) == ("repalign", 50, 3, 1)
    assert hash(p) == hash(RepeatCountParams("repalign", 50, 3, 1))  # lru_cache key (repeats.py:47)
    with pytest.raises(Exception):
        p.max_iters = 3  # frozen
    # strkit/call/repeat_count_params.py:17-42
    g = lambda cn: get_reference_rc_params("repalign", cn, 250)
    assert (g(10).max_iters, g(10).initial_step_size, g(10).initial_local_search_range) == (250, 1, 3)
    assert (g(199).max_iters, g(199).initial_step_size) == (250, 1)
    assert (g(200).max_iters, g(200).initial_step_size, g(200).initial_local_search_range) == (200, 3, 3)
    assert (g(999).max_iters, g(999).initial_step_size) == (200, 3)
    assert (g(1000).max_iters, g(1000).initial_step_size) == (150, 5)
    assert (g(1999).max_iters, g(1999).initial_step_size) == (150, 5)
    assert (g(2000).max_iters, g(2000).initial_step_size, g(2000).initial_local_search_range) == (50, 15, 1)


def test_synthetic_generator_is_deterministic_and_shaped():
    a, b = make_config(2, n_loci=20), make_config(2, n_loci=20)
    assert np.array_equal(a.seqs, b.seqs) and np.array_equal(a.est_cn, b.est_cn)
    assert not np.array_equal(a.seqs[:1000], make_config(2, n_loci=20, seed_shift=1).seqs[:1000])
    assert a.n_loci == 20 and a.n_reads == 20 * CONFIGS[2]["reads_per_locus"]
    assert (a.seq_off[1:] - a.seq_off[:-1] == a.nfl + a.ntr + a.nfr).all()
    for l in range(a.n_loci):
        assert 3 <= len(a.motif(l)) <= 6
    fl, tr, fr = a.read(0)
    assert 60 <= len(fl) <= 80 and 60 <= len(fr) <= 80
    assert a.algorithmic_bytes() == int(a.seq_off[-1]) + 16 * a.n_reads + int(a.motif_off[-1]) + 8 * a.n_loci
    s = a.locus_slice(5, 9)
    assert s.n_loci == 4 and s.read(0) == a.read(int(a.read_off[5])) and s.motif(3) == a.motif(8)


def test_sharding_partitions_loci_and_is_balanced():
    from strkit_amd.sharding import deal_blocks, select_loci
    b = make_config(3, n_loci=90)
    for world in (1, 2, 3, 8):
        shares = deal_blocks(b, world, block=7)
        allv = np.sort(np.concatenate(shares))
        assert np.array_equal(allv, np.arange(b.n_loci))  # every locus exactly once
        if world > 1:
            loads = [sum(int(b.read_off[l + 1] - b.read_off[l]) for l in s) for s in shares]
            assert max(loads) <= 1.5 * (sum(loads) / world) + 7 * 20
    sub, reads = select_loci(b, deal_blocks(b, 2, block=7)[1])
    for i, r in enumerate(reads[:50]):
        assert sub.read(i) == b.read(int(r))
    assert sub.n_reads == len(reads) and sub.n_loci == len(deal_blocks(b, 2, block=7)[1])


def _gloo_worker(rank, world, port, q):
    import torch.distributed as dist
    from strkit_amd.sharding import count_loci_sharded
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    b = make_config(1, n_loci=30)
    full = count_loci_sharded(b, oracle_count, device=None, block=4)  # the oracle stands in for the GPU on CPU
    q.put((rank, {k: v.tolist() for k, v in full.items()}))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_gather_equals_single_process():
    """world_size-2 gloo: sharding + one all-gather reproduce the 1-process table bit for bit."""
    import socket

    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    exp = oracle_count(make_config(1, n_loci=30))
    for rank in (0, 1):
        for k, v in exp.items():
            assert got[rank][k] == v.tolist()


def test_aligned_pair_matches_from_cigar():
    from strkit_amd.realign import cigar_to_string, get_aligned_pair_matches
    enc = {"M": 0, "I": 1, "D": 2, "=": 7, "X": 8}
    cig = np.array([(n << 4) | enc[o] for n, o in [(3, "D"), (2, "="), (1, "I"), (1, "X"), (2, "D"), (2, "=")]], np.uint32)
    assert cigar_to_string(cig) == "3D2=1I1X2D2="
    ac = get_aligned_pair_matches(cig, 100, 0, swap=True)      # "query" = ref window at 100, "ref" = read at 0
    assert ac.ref_coords.tolist() == [100, 101, 103, 104, 105]
    assert ac.query_coords.tolist() == [3, 4, 5, 8, 9]
    ac2 = get_aligned_pair_matches(cig, 100, 0)
    assert ac2.query_coords.tolist() == ac.ref_coords.tolist() and len(ac2) == 5 and ac2.pair_at_idx(2) == (103, 5)


def test_adjusted_score_and_read_filters_follow_the_callers_loop():
    """call_locus.py:1172,1222-1252 restated as a plain loop vs the vectorised host helper."""
    from strkit_amd.batch import calc_adj_score, filter_reads
    from strkit_amd.synth import make_config
    b = make_config(2, n_loci=40)
    rng = np.random.default_rng(4)
    total = (b.nfl + b.ntr + b.nfr).astype(np.int64)
    score = (2 * total).astype(np.int32)                       # perfect reads: adj 2.0 (docs/output_formats.md:102)
    assert np.allclose(calc_adj_score(score, b.nfl, b.ntr, b.nfr), 2.0)
    bad = rng.random(b.n_reads) < 0.12
    score[bad] = (total[bad] * rng.uniform(-1.0, 0.15, int(bad.sum()))).astype(np.int32)
    got = filter_reads(b, {"score": score})
    for l in range(b.n_loci):
        poor, ok = 0, True
        for r in range(int(b.read_off[l]), int(b.read_off[l + 1])):
            adj = score[r] / total[r]
            if not ok:
                assert not got["keep"][r]
                continue
            if adj < 0.1:
                if adj < 0.1:
                    poor += 1
                    if poor > 3:
                        ok = False
                assert not got["keep"][r]
                continue
            assert got["keep"][r] and abs(got["sc"][r] - adj) < 1e-12
        assert bool(got["locus_ok"][l]) == ok
    assert (~got["locus_ok"]).any() and got["locus_ok"].any()


def _gloo_call_worker(rank, world, port, q):
    import torch.distributed as dist
    from strkit_amd.frontend.call import call_blocks_sharded
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    ref = FakeRef()

    def fake_call(mine):
        rows, n, tm = fake_rows(mine, ref)
        return rows, n, {**tm, "count_s": 0.1 * (rank + 1)}

    merged, n, tm = call_blocks_sharded(gloo_blocks(), fake_call, ref)
    q.put((rank, merged, n, tm))
    dist.barrier()
    dist.destroy_process_group()


def test_call_driver_shards_locus_blocks_over_two_ranks():
    """world_size-2 gloo: blocks are dealt to ranks, fixed-size per-locus / per-read records (names as a fixed-width field)
    are all-gathered, and every rank ends with the rows a single process builds, in catalog order."""
    import socket

    import torch.multiprocessing as mp
    from strkit_amd.frontend.call import deal_locus_blocks
    from strkit_amd.frontend.loci import Locus
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gloo_call_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = [q.get(timeout=60) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want_rows, want_n, want_tm = fake_rows(gloo_blocks(), FakeRef())
    want_rows.sort(key=lambda r: r["locus_index"])
    assert any(len(nm) > 64 for r in want_rows for nm in (r.get("reads") or {}))       # a name longer than the default field
    for rank, merged, n, tm in got:
        assert merged == want_rows and n == want_n
        assert [e["locus_index"] for e in tm["errors"]] == [e["locus_index"] for e in want_tm["errors"]] != []
        assert abs(tm["count_s"] - 0.2) < 1e-9
    blocks = [[Locus(i + 1, "x", "chr1", 0, 100 * (i + 1), "CAG")] for i in range(7)]
    shares = deal_locus_blocks(blocks, 3)
    assert sorted(k for s_ in shares for k in s_) == list(range(7)) and shares == deal_locus_blocks(blocks, 3)
    assert shares[0][-1] == 6     # the heaviest block goes to the first rank


def _gloo_stage_worker(rank, world, port, q):
    """The staging / gather layout of `bench.py --strong`, on CPU tensors over gloo (the oracle stands in for the GPU)."""
    import torch
    import torch.distributed as dist
    from strkit_amd.sharding import NF, deal_blocks, gathered_step_table, select_loci, share_sizes, step_rows
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    catalog = make_config(2, n_loci=26)
    shares = deal_blocks(catalog, world, block=3)
    mine, my_reads = select_loci(catalog, shares[rank])
    rows, G = max(share_sizes(catalog, shares)), 3
    stage = torch.full((G * NF, rows), -1, dtype=torch.int32)
    stage[0::NF, :len(my_reads)] = torch.from_numpy(my_reads.astype(np.int32))
    res = oracle_count(mine)
    for j in range(G):                                     # G steps of one round (the same share every step)
        o = step_rows(stage, j)
        for i, k in enumerate(("cn", "score", "n_iters", "start")):
            o[1 + i, :mine.n_reads] = torch.from_numpy(res[k] + j * (k == "n_iters"))     # steps differ: the layout must not mix them
    gathered = torch.zeros((world * G * NF, rows), dtype=torch.int32)
    dist.all_gather_into_tensor(gathered, stage)
    q.put((rank, [gathered_step_table(gathered.numpy(), world, G, j, catalog.n_reads).tolist() for j in range(G)]))
    dist.barrier()
    dist.destroy_process_group()


def test_bench_strong_staging_layout_over_two_ranks():
    import socket

    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gloo_stage_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    exp = oracle_count(make_config(2, n_loci=26))
    for rank in (0, 1):
        for j in range(3):
            t = np.array(got[rank][j], np.int32)
            assert np.array_equal(t[0], exp["cn"]) and np.array_equal(t[1], exp["score"])
            assert np.array_equal(t[2], exp["n_iters"] + j) and np.array_equal(t[3], exp["start"])


def test_realign_i16_saturation_flags():
    """What parasail's fixed 16-bit kernel (realign.py:56) would have done: flags from lengths and 32-bit scores."""
    lib = _lib.load(build=False)
    s1 = np.array([0, 400, 400 + 16383, 400 + 16383 + 17000, 400 + 16383 + 17000 + 20000], np.int64)
    s2 = np.array([0, 15000, 40000, 70000, 70010], np.int64)      # the last read is 10 bases long
    score = np.array([790, 32000, 32766, 12], np.int32)
    out = np.full(4, -1, np.int32)
    assert lib.strk_realign_i16_flags(4, s1.ctypes.data, s2.ctypes.data, score.ctypes.data, out.ctypes.data) == 0
    assert out.tolist() == [0, _lib.STRK_I16_CELL_MAY_SATURATE,
                            _lib.STRK_I16_CELL_MAY_SATURATE | _lib.STRK_I16_SCORE_SATURATES, 0]
    assert lib.strk_realign_i16_flags(1, None, s2.ctypes.data, score.ctypes.data, out.ctypes.data) == -22


def test_contiguous_block_dealing_gives_every_rank_one_balanced_run():
    """The file path deals ONE run of consecutive catalog blocks to every rank (a rank then loads only its own byte range of the
    alignment file), balanced by the same cost estimate as the scatter of the counting path."""
    from strkit_amd.frontend.call import deal_locus_blocks
    from strkit_amd.frontend.loci import Locus
    rng = np.random.default_rng(9)
    blocks = []
    pos = 1000
    for b in range(57):
        blk = []
        for _ in range(int(rng.integers(1, 200))):
            n = int(rng.integers(6, 400))
            blk.append(Locus(len(blk), f"l{b}_{len(blk)}", "chr1", pos, pos + n, "CAG", 70))
            pos += n + 500
        blocks.append(blk)
    cost = [sum((l.right_coord - l.left_coord + 140) ** 2 for l in blk) for blk in blocks]
    for world in (1, 2, 3, 8):
        runs = deal_locus_blocks(blocks, world, contiguous=True)
        assert sorted(k for r in runs for k in r) == list(range(len(blocks)))
        for r in runs:
            assert r == list(range(r[0], r[-1] + 1)) if r else True          # one run of consecutive blocks
        assert [r[0] for r in runs if r] == sorted(r[0] for r in runs if r)  # in catalog order over the ranks
        share = sum(cost) / world
        assert max(sum(cost[k] for k in r) for r in runs) < share + max(cost), world
    # the scatter (counting path) stays what it was: every block exactly once
    assert sorted(k for r in deal_locus_blocks(blocks, 3) for k in r) == list(range(len(blocks)))


def test_class_known_band_geometry_equals_the_search_over_the_classes(tmp_path):
    """band_geometry_of_class (what the band kernels recompute per item from its class) must give exactly what band_geometry
    (k_plan: the search over the eight classes) gave for every eligible item: same band, same column range.  Host build of
    strk_search.h, 3 million random shapes incl. long windows, every window half-width and every band placement (BandTune)."""
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        pytest.skip("no host C++ compiler")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "geo_check.cpp"
    src.write_text(r"""
#include <cstdio>
#include <random>
#include <algorithm>
#include "%s/strkit_amd/csrc/strk_search.h"
int main() {
    std::mt19937 rng(7);
    long n_ok = 0, bad = 0, fly_limits = 0;
    for (long it = 0; it < 3000000; ++it) {
        int nfl = 1 + rng() %% 260, nfr = 1 + rng() %% 127, m = 1 + rng() %% ((rng() %% 8 == 0) ? 200 : 24);
        int est = rng() %% ((rng() %% 4 == 0) ? 2100 : 60);
        int W = 3 + rng() %% 13;
        int lo = std::max(0, est - W), n = std::min(32, est + W - lo + 1);
        int ntr = std::max(0, est * m + (int)(rng() %% 41) - 20);
        strk::BandTune tune = {(int)(rng() %% 3 == 0 ? 64 : 3 + rng() %% 5), (int)(rng() %% 2 ? 0 : rng() %% 33)};
        strk::BandGeo a = strk::band_geometry(nfl, ntr, nfr, m, lo, n, tune);
        if (!a.ok) continue;
        ++n_ok;
        if (strk::band_class_fly(a.cls) && (nfl > strk::kBandFlyMaxFlank || m > strk::kBandFlyMaxMotif)) ++fly_limits;
        strk::BandGeo b = strk::band_geometry_of_class(a.cls, nfl, ntr, m, lo, n, tune);
        if (a.cls != b.cls || a.G != b.G || a.wd != b.wd || a.dlo != b.dlo || a.bwd != b.bwd || a.bdlo != b.bdlo ||
            a.cmin != b.cmin || a.ncol != b.ncol) ++bad;
    }
    printf("%%ld %%ld %%ld\n", n_ok, bad, fly_limits);
    return 0;
}
""" % root)
    exe = tmp_path / "geo_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", str(exe), str(src)], check=True)
    n_ok, bad, fly_limits = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert n_ok > 1_000_000 and bad == 0
    assert fly_limits == 0      # the on-the-fly classes never get a flank or a motif their staged 2 x 256 bytes cannot hold


def test_search_replay_with_every_narrowing_schedule_equals_a_plain_python_search(tmp_path):
    """Host build of strk_search.h::search_replay (the function the kernels and the window-miss path run) against the plain
    Python loop above on 20 000 random score tables: every schedule of local_search_range (STRK_NARROW_*), both tie rules,
    steps 1-5, ranges 0-5, small max_iters, starts inside and outside the table (window misses), flat tables (ties)."""
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        pytest.skip("no host C++ compiler")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "search_check.cpp"
    src.write_text(r"""
#include <cstdio>
#include <vector>
#include "%s/strkit_amd/csrc/strk_search.h"
struct Seen { std::vector<char> v; bool test(int k) const { return v[k]; } void set(int k) { v[k] = 1; } };
int main() {
    int start, step, lsr, max_iters, tie, narrow, lo, n;
    while (scanf("%%d %%d %%d %%d %%d %%d %%d %%d", &start, &step, &lsr, &max_iters, &tie, &narrow, &lo, &n) == 8) {
        std::vector<int32_t> sc(n);
        for (int k = 0; k < n; ++k) scanf("%%d", &sc[k]);
        Seen seen; seen.v.assign(n, 0);
        strk::SearchResult r = strk::search_replay(start, step, lsr, max_iters, tie, sc.data(), lo, n, seen, narrow);
        if (r.miss) printf("miss\n"); else if (r.empty) printf("empty\n"); else printf("%%d %%d %%d\n", r.cn, r.score, r.n_explored);
    }
    return 0;
}
""" % root)
    exe = tmp_path / "search_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", str(exe), str(src)], check=True)
    from helpers import py_search
    rng = np.random.default_rng(20261009)
    lines, want = [], []
    for _ in range(20000):
        lo, n = int(rng.integers(0, 30)), int(rng.integers(1, 48))
        kind = int(rng.integers(4))
        peak = lo + int(rng.integers(-3, n + 3))
        if kind == 0:
            sc = rng.integers(-50, 400, size=n)
        elif kind == 1:                                        # one hill, noisy
            sc = 300 - 7 * np.abs(np.arange(lo, lo + n) - peak) + rng.integers(-6, 7, size=n)
        elif kind == 2:                                        # plateaus: ties decide
            sc = 300 - 10 * (np.abs(np.arange(lo, lo + n) - peak) // 3)
        else:
            sc = np.full(n, 17)
        start = lo + int(rng.integers(-4, n + 4))
        step, lsr = int(rng.integers(1, 6)), int(rng.integers(0, 6))
        max_iters, tie, narrow = int(rng.choice((1, 3, 7, 20, 50))), int(rng.integers(2)), int(rng.integers(4))
        lines.append(" ".join(str(int(x)) for x in (start, step, lsr, max_iters, tie, narrow, lo, n, *sc)))
        want.append(py_search(start, step, lsr, max_iters, tie, narrow, {lo + k: int(sc[k]) for k in range(n)}))
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.split("\n")
    seen_kinds = set()
    for k, (line, w) in enumerate(zip(out, want)):
        g = line if line in ("miss", "empty") else tuple(int(x) for x in line.split())
        assert g == w, (k, lines[k][:80], g, w)
        seen_kinds.add(w if isinstance(w, str) else "found")
    assert seen_kinds == {"miss", "found"} or seen_kinds == {"miss", "found", "empty"}


def test_adaptive_policies_follow_their_scripted_trajectories(tmp_path):
    """Host build of strk_policy.h (no HIP in it): the default-window policy, the band gate and the grid history driven through
    scripted call sequences.  The expected trajectories are the rules the host side has applied since round 4 (window levels
    +-4 5 6 8 11 15, start +-8, floor +-6 / +-8 for motifs of 1-2 bases; band cool-downs 32 .. 16 384; grids from the previous
    call's queue lengths with 50 % head-room), written out here by hand."""
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        pytest.skip("no host C++ compiler")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "policy_check.cpp"
    src.write_text(r"""
#include <cstdio>
#include <cstring>
#include "%s/strkit_amd/csrc/strk_policy.h"
// one command per line, one line of output per command:
//   w k reach               window of bucket k for local_search_range + step_size = reach
//   u k loci miss reps      `reps` finished calls with `loci` loci and `miss` window misses in bucket k; prints the +-window of k
//   r                       reset; prints the five windows
//   b reads fallbacks reps  band gate: `reps` finished calls; prints cooldown penalty probation
//   h prob bm reads exact wide long band_cells wide_cells    grid history of a finished call; prints valid tail_heavy
//   p mode bm chunks reads full                              predicted blocks
int main() {
    strk_policy::WindowPolicy win;
    strk_policy::BandGate gate;
    strk_policy::GridHistory hist;
    char cmd;
    long long a[8];
    while (scanf(" %%c", &cmd) == 1) {
        if (cmd == 'w') { scanf("%%lld %%lld", a, a + 1); printf("%%d\n", win.window((int)a[0], (int)a[1])); }
        else if (cmd == 'u') {
            scanf("%%lld %%lld %%lld %%lld", a, a + 1, a + 2, a + 3);
            for (long long i = 0; i < a[3]; ++i) win.update((int)a[0], (int)a[1], (int)a[2]);
            printf("%%d\n", win.window((int)a[0], 0));
        } else if (cmd == 'r') {
            win.reset();
            for (int k = 0; k < strk_policy::kWinBuckets; ++k) printf("%%d ", win.window(k, 0));
            printf("\n");
        } else if (cmd == 'b') {
            scanf("%%lld %%lld %%lld", a, a + 1, a + 2);
            for (long long i = 0; i < a[2]; ++i) gate.update((int)a[0], (int)a[1]);
            printf("%%d %%d %%d\n", gate.cooldown, gate.penalty, (int)gate.probation);
        } else if (cmd == 'h') {
            for (int i = 0; i < 8; ++i) scanf("%%lld", a + i);
            hist.update(a[0] != 0, (int)a[1], (int)a[2], (int)a[3], (int)a[4], (int)a[5], (uint64_t)a[6], (uint64_t)a[7]);
            printf("%%d %%d\n", (int)hist.valid, (int)hist.tail_heavy);
        } else if (cmd == 'p') {
            for (int i = 0; i < 5; ++i) scanf("%%lld", a + i);
            printf("%%d\n", hist.predicted_blocks(hist.usable((int)a[0], (int)a[1]), (int)a[2], (int)a[3], (int)a[4]));
        }
    }
    return 0;
}
""" % root)
    exe = tmp_path / "policy_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", str(exe), str(src)], check=True)
    script = []            # (command, expected output line)

    def step(cmd, want):
        script.append((cmd, " ".join(str(x) for x in want) if isinstance(want, (tuple, list)) else str(want)))

    QUIET, MID, MISS = "1000 1", "1000 3", "1000 5"     # misses <= loci / 1000 | in between | > max(1, loci / 250)
    # --- window -----------------------------------------------------------------------------------------------------------
    step("r", "8 8 8 8 8 ")
    for k in range(5):                                   # eight quiet calls: buckets 1-4 to +-6, bucket 0 stays at +-8
        step(f"u {k} {QUIET} 7", 8)
        step(f"u {k} {QUIET} 1", 8 if k == 0 else 6)
    step(f"u 0 {QUIET} 5000", 8)                         # ... and nothing below the bucket's floor
    step(f"u 1 {QUIET} 5000", 6)
    # a step down followed by a call with misses is a failed probe: up at once, and the next step down needs 64, 128 ... 4 096
    for failed in range(1, 10):
        step(f"u 1 {MISS} 1", 8)
        need = min(64 << (failed - 1), 4096)
        step(f"u 1 {QUIET} {need - 1}", 8)
        step(f"u 1 {QUIET} 1", 6)
    step("r", "8 8 8 8 8 ")                              # reset restores all of it: eight quiet calls are enough again
    step(f"u 1 {QUIET} 7", 8)
    step(f"u 1 {QUIET} 1", 6)
    step("r", "8 8 8 8 8 ")
    step(f"u 2 {MISS} 1", 11)                            # one level up per call with misses, up to +-15
    step(f"u 2 {MISS} 1", 15)
    step(f"u 2 {MISS} 1", 15)
    step("w 2 0", 15)
    step(f"u 2 {QUIET} 63", 15)                          # above the start level a step down needs 64 quiet calls
    step(f"u 2 {QUIET} 1", 11)
    step(f"u 2 {QUIET} 63", 11)
    step(f"u 2 {QUIET} 1", 8)
    step(f"u 2 {QUIET} 7", 8)                            # (these were no failed probes: from the start level, eight)
    step(f"u 2 {QUIET} 1", 6)
    step(f"u 3 {QUIET} 7", 8)                            # a call in between only zeroes the quiet count
    step(f"u 3 {MID} 1", 8)
    step(f"u 3 {QUIET} 7", 8)
    step(f"u 3 {QUIET} 1", 6)
    step("u 4 100 1 1", 8)                               # small calls: one miss of 100 loci is "in between", two are misses
    step("u 4 100 2 1", 11)
    step("r", "8 8 8 8 8 ")
    step(f"u 1 {QUIET} 7", 8)                            # a bucket with no loci in the call is not touched
    step("u 1 0 0 10", 8)
    step("u 1 0 5 10", 8)
    step(f"u 1 {QUIET} 1", 6)
    step("w 0 3", 8)                                     # never less than min(15, local_search_range + step_size)
    step("w 0 10", 10)
    step("w 0 20", 15)
    step("w 1 3", 6)
    step("w 1 7", 7)
    step("w 1 99", 15)
    # --- band gate --------------------------------------------------------------------------------------------------------
    step("b 63 63 1", (0, 32, 1))                        # starts on probation; fewer than 64 band reads change nothing
    step("b 0 0 5", (0, 32, 1))
    penalty = 32
    for _ in range(12):                                  # fall-backs > half: cool-down, probation, the next penalty doubled
        nxt = min(2 * penalty, 16384)
        step("b 64 33 1", (penalty, nxt, 1))
        step("b 1000 0 1", (penalty - 1, nxt, 1))        # a cool-down counts down one per call whatever the call held
        step(f"b 1000 1000 {penalty - 2}", (1, nxt, 1))
        step("b 10 0 1", (0, nxt, 1))
        penalty = nxt
    assert penalty == 16384
    step("b 64 32 1", (0, 32, 0))                        # a healthy call (half is not "more than half") ends probation
    step("b 63 63 1", (0, 32, 0))
    step("b 100 51 1", (32, 64, 1))
    # --- grid history -----------------------------------------------------------------------------------------------------
    step("p 0 1 100 1000 2000", 2000)                    # no history: the full grid
    step("h 1 1 1000 40 100 0 1000 300", (0, 1))         # a call on probation: invalid
    step("p 0 1 100 1000 2000", 2000)
    step("h 0 1 1000 40 100 0 1000 300", (1, 1))
    step("p 0 1 100 1000 2000", 39)                      # floor(100 * 1000 / 1000 * 1.5 / 4) + 2
    step("p 0 1 100 2000 2000", 77)
    step("p 0 1 100 0 2000", 2)                          # (an empty batch counts as one read)
    step("p 0 0 100 1000 2000", 2000)                    # another band mode
    step("p 1 1 100 1000 2000", 2000)                    # not a whole batched call
    step("p 0 1 0 1000 2000", 1)                         # an empty queue
    step("p 0 1 100000 1000 2000", 2000)                 # clamped to [1, full]
    step("p 0 1 100 1000 10", 10)
    step("h 0 0 0 4 4 4 1000 250", (1, 0))               # tail_heavy: each band kernel more than a quarter of the other's cells
    step("p 0 0 4 3 100", 6)                             # (hist_reads = max(1, n_reads))
    step("p 0 1 4 3 100", 100)
    step("h 0 1 10 0 0 0 1000 4001", (1, 0))
    step("h 0 1 10 0 0 0 1000 3999", (1, 1))
    step("h 0 1 10 0 0 0 251 1000", (1, 1))
    step("h 0 1 10 0 0 0 0 0", (1, 0))
    out = subprocess.run([str(exe)], input="\n".join(c for c, _ in script) + "\n", check=True, capture_output=True, text=True).stdout.split("\n")
    assert len(out) == len(script) + 1
    for k, ((cmd, want), got) in enumerate(zip(script, out)):
        assert got.rstrip() == want.rstrip(), (k, cmd, got, want)


def _check_groups_restated(max_group, max_len, n_groups, n_bytes, off, starts, lens):
    """strk_groups::check in plain Python: (rc, n_seqs, longest, sum, message); None stands for a NULL array."""
    def bad(msg):
        return (-22, 0, 0, 0, msg)
    if n_groups < 0:
        return bad("n_groups < 0")
    if n_bytes < 0:
        return bad("n_seq_bytes < 0")
    if n_groups == 0:
        return (0, 0, 0, 0, "")
    if off is None:
        return bad("NULL argument")
    if off[0] != 0:
        return bad("group_off[0] must be 0")
    for g in range(n_groups):
        n = off[g + 1] - off[g]
        if n < 0:
            return bad(f"group {g}: group_off is decreasing")
        if n > max_group:
            return bad(f"group {g}: {n} sequences (at most {max_group})")
    n_seqs = off[n_groups]
    if n_seqs > 0 and (starts is None or lens is None):
        return bad("NULL argument")
    for i in range(n_seqs):
        if lens[i] < 0 or lens[i] > max_len:
            return bad(f"sequence {i}: length {lens[i]} is outside 0..{max_len}")
        if starts[i] < 0 or starts[i] + lens[i] > n_bytes:
            return bad(f"sequence {i}: bytes {starts[i]}..{starts[i] + lens[i]} lie outside the {n_bytes} given")
    lens = (lens or [])[:n_seqs]
    return (0, n_seqs, max(lens, default=0), sum(lens), "")


def _cut_pieces_restated(costs, budget, max_items):
    """strk_groups::cut_piece over a whole list: in order while it fits, at least one item, at most max_items (None: no cap)."""
    pieces, p0 = [], 0
    while p0 < len(costs):
        p1, used, off = p0, 0, []
        while p1 < len(costs) and (max_items is None or p1 - p0 < max_items):
            if p1 > p0 and used + costs[p1] > budget:
                break
            off.append(used)
            used += costs[p1]
            p1 += 1
        pieces.append((p0, p1, used, off))
        p0 = p1
    return pieces


def test_group_view_checks_and_piece_cutting_equal_their_plain_restatement(tmp_path):
    """Host build of strk_groups.h (no HIP in it): the one check of a view of groups, and the cutting of a list into pieces by a
    workspace bound, over scripted cases; the expectation is the plain Python restatement above."""
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        pytest.skip("no host C++ compiler")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "groups_check.cpp"
    src.write_text(r"""
#include <cstdio>
#include <vector>
#include "%s/strkit_amd/csrc/strk_groups.h"
// one command per line, one line of output per command:
//   c max_group max_len n_groups n_seq_bytes n_off off... n_seqs start... len...   (n_off / n_seqs = -1: that array is NULL)
//       prints rc n_seqs max_len total_len message
//   p budget max_items n cost...    (max_items = -1: no cap)    prints every piece as "p0 p1 used off...;"
static long long rd() {
    long long x = 0;
    return scanf("%%lld", &x) == 1 ? x : 0;
}
int main() {
    char cmd;
    while (scanf(" %%c", &cmd) == 1) {
        if (cmd == 'c') {
            const long long max_group = rd(), max_len = rd(), n_groups = rd(), n_bytes = rd(), n_off = rd();
            // arrays of exactly the size given, so that a read past an end is one a sanitizer build sees
            std::vector<int32_t> off(n_off < 0 ? 0 : (size_t)n_off);
            for (auto& o : off) o = (int32_t)rd();
            const long long n_seqs = rd();
            std::vector<int64_t> start(n_seqs < 0 ? 0 : (size_t)n_seqs);
            std::vector<int32_t> len(start.size());
            for (auto& x : start) x = rd();
            for (auto& x : len) x = (int32_t)rd();
            strk_groups::View v{(int32_t)n_groups, n_off < 0 ? nullptr : off.data(), n_bytes, n_seqs < 0 ? nullptr : start.data(),
                                n_seqs < 0 ? nullptr : len.data()};
            strk_groups::Totals t;
            strk_groups::Message m;
            m.text[0] = 0;
            const int rc = strk_groups::check(v, (int)max_group, (int)max_len, &t, &m);
            printf("%%d %%d %%d %%lld %%s\n", rc, t.n_seqs, t.max_len, (long long)t.total_len, rc ? m.text : "");
        } else if (cmd == 'p') {
            const long long budget = rd(), max_items = rd(), n = rd();
            std::vector<int64_t> cost((size_t)n), off;
            for (auto& x : cost) x = rd();
            for (size_t p0 = 0, p1; p0 < cost.size(); p0 = p1) {
                int64_t used = -1;
                p1 = strk_groups::cut_piece(p0, cost.size(), [&](size_t p) { return cost[p]; }, budget,
                                            max_items < 0 ? strk_groups::kNoItemCap : (size_t)max_items, off, &used);
                printf("%%zu %%zu %%lld", p0, p1, (long long)used);
                for (int64_t o : off) printf(" %%lld", (long long)o);
                printf(";");
            }
            printf("\n");
        }
    }
    return 0;
}
""" % root)
    exe = tmp_path / "groups_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", str(exe), str(src)], check=True)
    script = []            # (command, expected output line)

    def view(n_groups, n_bytes, off, starts, lens, max_group=250, max_len=65535):
        cmd = [max_group, max_len, n_groups, n_bytes, -1 if off is None else len(off), *(off or []),
               -1 if starts is None else len(starts), *(starts or []), *(lens or [])]
        rc, n_seqs, longest, total, msg = _check_groups_restated(max_group, max_len, n_groups, n_bytes, off, starts, lens)
        script.append(("c " + " ".join(str(x) for x in cmd), f"{rc} {n_seqs} {longest} {total} {msg}".rstrip()))
        return rc, n_seqs, longest, total

    assert view(3, 20, [0, 2, 2, 5], [0, 3, 9, 9, 15], [3, 6, 0, 6, 5]) == (0, 5, 6, 20)     # a good view, slices end to end
    assert view(0, 0, None, None, None) == (0, 0, 0, 0)                                      # no groups: nothing is looked at
    assert view(0, 7, [5], [-1], [-1]) == (0, 0, 0, 0)
    assert view(-1, 0, [0], [], [])[0] == -22
    assert view(1, -1, [0, 0], [], [])[0] == -22
    assert view(2, 9, None, [0], [1])[0] == -22                                              # NULL group_off
    assert view(2, 9, [1, 2, 3], [0, 1, 2], [1, 1, 1])[0] == -22                             # group_off[0] != 0
    assert view(3, 9, [0, 2, 1, 3], [0, 1, 2], [1, 1, 1])[0] == -22                          # decreasing offsets
    assert view(1, 300, [0, 251], [0] * 251, [1] * 251)[0] == -22                            # a group of 251
    assert view(1, 300, [0, 250], [0] * 250, [1] * 250) == (0, 250, 1, 250)                  # ... and of 250
    assert view(2, 9, [0, 1, 4], [0, 0, 0, 0], [3, 3, 3, 3], max_group=2)[0] == -22          # the limit is the caller's
    assert view(1, 9, [0, 1], [0], [-1])[0] == -22                                           # a length of -1
    assert view(1, 70000, [0, 1], [0], [65536])[0] == -22                                    # ... of 65 536
    assert view(1, 70000, [0, 1], [0], [65535]) == (0, 1, 65535, 65535)                      # ... of 65 535
    assert view(1, 70000, [0, 1], [0], [4097], max_len=4096)[0] == -22
    assert view(1, 9, [0, 1], [-1], [3])[0] == -22                                           # a start of -1
    assert view(2, 9, [0, 1, 2], [0, 7], [3, 3])[0] == -22                                   # one byte past n_seq_bytes
    assert view(2, 9, [0, 1, 2], [0, 6], [3, 3]) == (0, 2, 3, 6)                             # ending exactly at it
    assert view(1, 0, [0, 2], [0, 0], [0, 0]) == (0, 2, 0, 0)                                # empty strings of an empty buffer
    assert view(1, 0, [0, 1], [1], [0])[0] == -22
    assert view(1, 2 ** 40, [0, 1], [2 ** 40 - 5], [5]) == (0, 1, 5, 5)                      # 64-bit offsets
    assert view(1, 2 ** 40, [0, 1], [2 ** 62], [5])[0] == -22
    assert view(1, 9, [0, 2], None, None)[0] == -22                                          # NULL seq_start, sequences present
    assert view(2, 9, [0, 0, 0], None, None) == (0, 0, 0, 0)                                 # ... and none present
    assert view(5, 9, [0, 0, 2, 2, 2, 3], [0, 2, 4], [2, 2, 5]) == (0, 3, 5, 9)              # empty groups between full ones
    assert len({want.split(" ", 4)[-1] for _c, want in script if want.startswith("-22")}) >= 10   # every refusal has its own text

    def cut(costs, budget, max_items=None):
        pieces = _cut_pieces_restated(costs, budget, max_items)
        script.append((f"p {budget} {-1 if max_items is None else max_items} {len(costs)} " + " ".join(str(c) for c in costs),
                       "".join(" ".join(str(x) for x in (p0, p1, used, *off)) + ";" for p0, p1, used, off in pieces)))
        return [(p0, p1) for p0, p1, _u, _o in pieces]

    assert cut([9, 8, 7, 100], 5) == [(0, 1), (1, 2), (2, 3), (3, 4)]                        # every item beyond the budget: alone
    assert cut([1, 2, 3, 4], 10) == [(0, 4)]                                                 # everything fits (exactly)
    assert cut([1, 2, 3, 4], 9) == [(0, 3), (3, 4)]
    assert cut([1] * 10, 100, 4) == [(0, 4), (4, 8), (8, 10)]                                # the item cap binds before the budget
    assert cut([1] * 10, 3, 4) == [(0, 3), (3, 6), (6, 9), (9, 10)]                          # ... and the budget before the cap
    assert cut([], 10) == [] and cut([], 10, 3) == []                                        # an empty range: no piece
    assert cut([0, 0, 50, 0, 60, 0], 100, 3) == [(0, 3), (3, 6)]                             # items that cost nothing
    assert cut([4, 100, 4, 4, 100, 100, 1], 8) == [(0, 1), (1, 2), (2, 4), (4, 5), (5, 6), (6, 7)]
    assert cut([2 ** 40, 2 ** 40, 1], 2 ** 41) == [(0, 2), (2, 3)]                           # 64-bit sums
    assert _cut_pieces_restated([5, 6, 7], 18, None) == [(0, 3, 18, [0, 5, 11])]             # offsets are the running sums
    assert cut([5, 6, 7, 9, 2], 18, 4) == [(0, 3), (3, 5)] and script[-1][1] == "0 3 18 0 5 11;3 5 11 0 9;"   # ... the program's too

    commands = tmp_path / "groups_check.in"      # (a file, so that the same run can be repeated by hand under a sanitizer build)
    commands.write_text("\n".join(c for c, _ in script) + "\n")
    out = subprocess.run([str(exe)], stdin=commands.open(), check=True, capture_output=True, text=True).stdout.split("\n")
    assert len(out) == len(script) + 1
    for k, ((cmd, want), got) in enumerate(zip(script, out)):
        assert got.rstrip() == want.rstrip(), (k, cmd[:80], got, want)


def test_allele_call_checkers_accept_and_refuse_what_they_should(tmp_path):
    """Host build of tools/phase_asan.cpp (no HIP in strk_alleles_check.h and strk_phase_check.h): the input checks of
    strk_call_alleles and strk_call_alleles_phased over random valid calls and every refusal, arrays of exactly their length;
    the program counts its own failures and exits 0 without one."""
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "phase_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tools", "phase_asan.cpp")], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert " 0 failed" in run.stdout, run.stdout


def test_realign_planner_accepts_refuses_and_lays_out_what_it_should(tmp_path):
    """Host build of tools/realign_asan.cpp (no HIP in strk_realign_plan.h): strk_realign's input check over every refusal, by
    its message, and the invariants of the plan (chunks, order, trace / edge / CIGAR ranges) over random valid calls and trace
    budgets from 1 MiB up, arrays of exactly their length; the gap-cost bound 2*open + (n1 - 2)*extend < 2^24 at the last
    (open, extend, n1) taken and the first refused along each of the three, and at n1 = 2^20; the program counts its own
    failures and exits 0 without one."""
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "realign_plan"
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tools", "realign_asan.cpp")], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert " 0 failed" in run.stdout, run.stdout
