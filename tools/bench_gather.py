"""What the record gather of a torch.distributed `call` costs (frontend/gather.py).

  python tools/bench_gather.py codec [--tree DIR]     encode + decode in process, no collective, on synthetic rows of 10 000 loci
                                                      x 30 reads: with call_alleles, consensus and count_kmers="peak", and the same
                                                      rows stripped to their read records.  --tree DIR imports strkit_amd from
                                                      another checkout (the parent commit's, for the baseline of the stripped rows:
                                                      there only _encode_rows / _decode_rows exist, and only they are timed).
  python tools/bench_gather.py ranks [--loci N]       GPU: one process, then two ranks over gloo on device 0, on a synthetic
                                                      alignment file with genotypes; prints gather_s, report_s and the wall time.

Three repeats each; every figure is printed, none is judged here."""
import argparse
import json
import os
import sys
import time

import numpy as np


def synthetic_rows(n_loci=10000, n_reads=30, calls=True, seed=1):
    """Rows of the shape `call --call-alleles --consensus --count-kmers peak` writes (two alleles, 15 reads each, sequences of
    24 to 200 bases, 3 or 5 k-mers per peak), or stripped to their read records; and the catalog and reference they need."""
    from strkit_amd.frontend.block import _locus_row
    from strkit_amd.frontend.loci import Locus
    from strkit_amd.frontend.options import CallOptions
    rng = np.random.default_rng(seed)
    genome = "".join(rng.choice(list("ACGT"), 4096))

    class Ref:
        def fetch(self, contig, a, b):
            return genome[a % 2048:a % 2048 + (b - a)]

    ref, opts, rows, loci = Ref(), CallOptions(), [], {}
    cns = rng.integers(8, 40, size=(n_loci, 2))
    ws = rng.random((n_loci, n_reads))
    for i in range(n_loci):
        motif = "CAG" if i % 3 else "GGCCT"
        locus = Locus(i + 1, f"l{i}", "chr1", 1000 + 200 * i, 1000 + 200 * i + 30, motif)
        loci[locus.t_idx] = locus
        a, b = sorted(int(c) for c in cns[i])
        reads = {f"m64011_190830_220126/{i * n_reads + k}/ccs": {"s": "+-"[k % 2], "cn": (a, b)[k % 2], "w": float(ws[i, k]), "sc": 0.9 + 0.001 * k, "sl": 3 * (a, b)[k % 2]}
                 for k in range(n_reads)}
        rd = {"ref_cn": 10, "left_coord_adj": locus.left_coord, "right_coord_adj": locus.right_coord,
              "ref_seq": ref.fetch("chr1", locus.left_coord, locus.right_coord), "ref_left_flank_seq": ref.fetch("chr1", locus.left_coord - 5, locus.left_coord)}
        row = _locus_row(locus, rd, reads, opts)
        if calls:
            for k, r in enumerate(reads.values()):
                r["p"] = k % 2
            kmers = [{motif[j:] + motif[:j]: int(c) * 15 - j for j in range(len(motif))} for c in (a, b)]
            row.update({"assign_method": "dist", "call": [a, b], "call_95_cis": [[a, a], [b, b + 1]], "call_99_cis": [[a - 1, a], [b, b + 1]],
                        "peaks": {"means": [a + 0.01, b - 0.02], "weights": [0.5, 0.5], "stdevs": [0.1, 0.2], "modal_n": 2, "n_reads": [15, 15],
                                  "seqs": [[motif * a, "single"], [motif * b, "best_rep"]], "start_anchor_seqs": [["ACGTA", "single"], ["ACGTA", "single"]],
                                  "kmers": kmers},
                        "read_peaks_called": True})
            row["mean_model_align_score"] = 0.9145
        rows.append(row)
    return rows, loci, ref


def _repeat(fn, n=3):
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def codec(args):
    from strkit_amd.frontend import gather as G
    new = hasattr(G, "_encode_calls")
    print(f"# codec: strkit_amd from {os.path.dirname(os.path.dirname(G.__file__))} ({'with' if new else 'without'} call tables)")
    for name, calls in (("rows with calls, sequences and peak k-mers", True), ("rows stripped to their read records", False)):
        rows, loci, ref = synthetic_rows(calls=calls)
        text = json.dumps(sorted(rows, key=lambda r: r["locus_index"]))
        if new:
            def both():
                got, _ = G._decode_shares(loci, ref, False, [G._encode_rows(rows, [])], [G._encode_calls(rows)])
                return got
            n_bytes = sum(t.nbytes for t in G._encode_rows(rows, [])) + sum(t.nbytes for t in G._encode_calls(rows).values())
        elif not calls:
            def both():
                got, _ = G._decode_rows(loci, ref, False, *G._encode_rows(rows, []))
                return got
            n_bytes = sum(t.nbytes for t in G._encode_rows(rows, []))
        else:
            print(f"{name}: not measured (this tree cannot encode them)")
            continue
        assert json.dumps(both()) == text
        ts = _repeat(both)
        print(f"{name}: 10 000 loci x 30 reads, {n_bytes / 1e6:.1f} MB of tables, encode + decode "
              f"{' / '.join(f'{t:.3f}' for t in ts)} s (spread {max(ts) - min(ts):.3f} s)")


def _rank(rank, world, port, paths, kw, q):
    os.environ["STRKIT_AMD_DEVICE"] = "0"
    import torch.distributed as dist
    from strkit_amd.frontend import call_sample
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    out = []
    for _ in range(3):
        dist.barrier()
        rep = call_sample(paths["bam"], paths["ref"], paths["loci"], **kw)
        out.append({"runtime": rep["runtime"], **{k: rep["stage_times"].get(k) for k in ("gather_s", "report_s", "alleles_s", "consensus_s", "kmers_s")},
                    "results": json.dumps(rep["results"]) if len(out) == 0 else None})
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def ranks(args):
    import socket
    import tempfile

    import torch.multiprocessing as mp
    from strkit_amd.frontend import call_sample
    from strkit_amd.frontend.synth_large import make_dataset_large
    kw = dict(call_alleles=True, consensus=True, count_kmers="peak", seed=7, processes=8, front_end="device")
    with tempfile.TemporaryDirectory() as d:
        t = make_dataset_large(d, n_loci=args.loci, depth=30, read_len=args.read_len, seed=3, procs=16)
        print(f"# ranks: {args.loci} loci x 30 reads of {args.read_len} bases, call_alleles + consensus + count_kmers=peak, device front end")
        one = [call_sample(t["paths"]["bam"], t["paths"]["ref"], t["paths"]["loci"], **kw) for _ in range(3)]
        print("one process: wall " + " / ".join(f"{r['runtime']:.3f}" for r in one) + " s, report_s "
              + " / ".join(f"{r['stage_times'].get('report_s', 0):.3f}" for r in one) + " s")
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        ctx = mp.get_context("spawn")
        q = ctx.Queue()
        procs = [ctx.Process(target=_rank, args=(r, 2, port, t["paths"], kw, q)) for r in range(2)]
        for p in procs:
            p.start()
        got = dict(q.get(timeout=600) for _ in procs)
        for p in procs:
            p.join(timeout=60)
            if p.exitcode != 0:
                sys.exit(f"a rank ended with {p.exitcode}")
        for rank in (0, 1):
            runs = got[rank]
            same = runs[0]["results"] == json.dumps(one[0]["results"])
            print(f"rank {rank} of 2 (one GPU): rows {'identical to' if same else 'DIFFERENT FROM'} one process; " + "; ".join(
                f"{k} " + " / ".join("-" if r[k] is None else f"{r[k]:.3f}" for r in runs) + " s" for k in ("runtime", "gather_s", "report_s", "alleles_s", "consensus_s", "kmers_s")))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("codec", "ranks"))
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--loci", type=int, default=2000)
    ap.add_argument("--read-len", type=int, default=3000)
    a = ap.parse_args()
    sys.path.insert(0, a.tree)
    {"codec": codec, "ranks": ranks}[a.mode](a)
