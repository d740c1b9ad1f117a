"""`strkit mi` for this project's own call files: Mendelian inheritance and the de novo test of a child / mother / father trio
(DESIGN.md §16).  Stands where the reference runs strkit/mi/base.py (trio assembly, rates), strkit/mi/strkit.py
(StrKitJSONCalculator, StrKitVCFCalculator) and strkit/mi/result.py (the per-locus rule, the corrections for multiple testing,
the report).  The per-locus rule runs in the library: strk_mi_trio on the device, strk_mi_trio_host on the host's cores; what
is here reads the files, packs the arrays, corrects for multiple testing in numpy and writes the report."""
from __future__ import annotations

import ctypes as C
import gzip
import json
import logging
import math
import re
from dataclasses import dataclass, field

import numpy as np

from . import _lib

__all__ = ["KINDS", "TESTS", "MT_METHODS", "FROM_NAMES", "DEFAULT_SEED", "TrioMember", "TrioArrays", "mi_trio_batch", "pack_loci",
           "load_trio_json", "load_trio_vcf", "assemble_trio", "correct_for_multiple_testing", "mi_result", "write_report_json",
           "locus_tsv", "summary_text", "histogram_text", "report_object", "run_mi"]

KINDS = ("strict", "pm1", "ci_95", "ci_99", "seq", "sl", "sl_pm1")
TESTS = {"none": _lib.STRK_MI_TEST_NONE, "x2": _lib.STRK_MI_TEST_X2, "wmw": _lib.STRK_MI_TEST_WMW, "wmw-gt": _lib.STRK_MI_TEST_WMW_GT}
FROM_NAMES = ("none", "?", "mat", "pat", "both")
CONFIGS = ((0, 0), (0, 1), (1, 0), (1, 1))
MT_METHODS = ("none", "bonferroni", "sidak", "holm-sidak", "holm", "simes-hochberg", "fdr_bh", "fdr_by")
SEX_CHROMOSOMES = frozenset(("chrX", "X", "chrY", "Y"))
# The reference shuffles the reads of a one-peak locus with an unseeded generator (strkit/mi/strkit.py:163); this project's
# choice is numpy's default_rng([seed, ordinal of the locus in its file]) with this default seed.
DEFAULT_SEED = 2718

log = logging.getLogger("strkit_amd.mi")


def _i32(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a if shape is None else a.reshape(shape)


def small_threshold() -> int:
    """Reads (all six groups together) of the largest locus k_mi_small takes; a larger one goes to k_mi_large."""
    out = (C.c_int32 * 3)()
    _lib.load().strk_mi_constants(out)
    return int(out[0])


def mi_trio_batch(gt, ci95, grp_off=None, cn=None, ci99=None, seq_id=None, seq_len=None, *, test: str = "none", sig_level: float = 0.05,
                  widen: float = 0.0, device: str = "gpu", ctx=None, piece_loci: int = 0, ws_budget: int = 0, _force_large: bool = False) -> dict:
    """The per-locus rule over packed arrays (include/strkit_amd.h: strk_mi_trio).  device="gpu": strk_mi_trio; "host":
    strk_mi_trio_host (no device is touched).  Returns respects int8 [n, 7] (1, 0, -1 = None) and, with a test, p float64 (NaN =
    not tested), config, mutation_from and status int32 [n]; "stats" for the device."""
    if test not in TESTS:
        raise ValueError(f"unknown test {test!r}")
    if device not in ("gpu", "host"):
        raise ValueError(f"device must be 'gpu' or 'host', not {device!r}")
    gt = _i32(gt, (-1, 6))
    n = gt.shape[0]
    ci95 = _i32(ci95, (n, 12))
    ci99 = None if ci99 is None else _i32(ci99, (n, 12))
    seq_id = None if seq_id is None else _i32(seq_id, (n, 6))
    seq_len = None if seq_len is None else _i32(seq_len, (n, 6))
    if grp_off is not None:
        grp_off = np.ascontiguousarray(grp_off, dtype=np.int64)
        if grp_off.size != 6 * n + 1:
            raise ValueError("grp_off must have 6 n + 1 entries")
    cn = None if cn is None else _i32(cn)
    p = _lib.MiParams(TESTS[test], int(piece_loci), float(sig_level), float(widen), int(ws_budget), int(bool(_force_large)), 0)
    out = {"respects": np.full((n, 7), -1, np.int8), "p": np.full(n, np.nan), "config": np.full(n, -1, np.int32),
           "mutation_from": np.zeros(n, np.int32), "status": np.zeros(n, np.int32)}
    args = [n, _lib.ptr(grp_off), _lib.ptr(cn), 0 if cn is None else int(cn.size), _lib.ptr(gt), _lib.ptr(ci95), _lib.ptr(ci99),
            _lib.ptr(seq_id), _lib.ptr(seq_len), C.byref(p), _lib.ptr(out["respects"]), _lib.ptr(out["p"]), _lib.ptr(out["config"]),
            _lib.ptr(out["mutation_from"]), _lib.ptr(out["status"])]
    L = _lib.load()
    if device == "host":
        _lib.check(L.strk_mi_trio_host(*args))
    else:
        ctx = ctx or _lib.default_context()
        stats = _lib.StrkStats()
        _lib.check(L.strk_mi_trio(ctx.handle, *args, C.byref(stats)))
        out["stats"] = stats.as_dict()
    return out


def pack_loci(loci) -> dict:
    """Loci as dicts (gt: six ints; ci95: six (lo, hi); optional ci99, seqs: six strings or None, reads: six sequences of ints)
    into the arrays mi_trio_batch takes.  The six strings of a locus are interned to the ids 0..5 of their first occurrences."""
    n = len(loci)
    gt = np.array([l["gt"] for l in loci], np.int32).reshape(n, 6)
    ci95 = np.array([l["ci95"] for l in loci], np.int32).reshape(n, 12)
    has99 = n > 0 and all(l.get("ci99") is not None for l in loci)
    ci99 = np.array([l["ci99"] for l in loci], np.int32).reshape(n, 12) if has99 else None
    seq_id = seq_len = None
    if any(l.get("seqs") is not None for l in loci):
        seq_id, seq_len = np.full((n, 6), -1, np.int32), np.zeros((n, 6), np.int32)
        for i, l in enumerate(loci):
            if l.get("seqs") is not None:
                seq_id[i], seq_len[i] = intern_seqs(l["seqs"])
    grp_off = cn = None
    if n > 0 and all("reads" in l for l in loci):
        sizes = np.array([len(g) for l in loci for g in l["reads"]], np.int64)
        grp_off = np.zeros(6 * n + 1, np.int64)
        np.cumsum(sizes, out=grp_off[1:])
        cn = np.fromiter((v for l in loci for g in l["reads"] for v in g), np.int32, int(grp_off[-1]))
    return {"gt": gt, "ci95": ci95, "ci99": ci99, "seq_id": seq_id, "seq_len": seq_len, "grp_off": grp_off, "cn": cn}


def intern_seqs(seqs):
    first: dict[str, int] = {}
    return [first.setdefault(s, len(first)) for s in seqs], [len(s) for s in seqs]


# ---- the files -----------------------------------------------------------------------------------------------------------------
@dataclass
class TrioMember:
    """One member's call file: every locus in file order as key -> record, a record being None (no call) or a dict of
    call (tuple of ints), cis (tuple of (lo, hi)), reads (tuple of tuples of ints), ref_cn, seqs (tuple of str or None), ps (bool)."""
    loci: dict = field(default_factory=dict)
    contigs: set = field(default_factory=set)
    has_seqs: bool = False


def split_reads_json(res: dict, rng) -> tuple:
    """get_read_counts (strkit/mi/strkit.py:146-172) with this project's seeded shuffle; the condition's precedence is the
    reference's, as written."""
    cns, peaks = [], []
    for r in res["reads"].values():
        if (pk := r.get("p")) is None:
            continue
        cns.append(r["cn"])
        peaks.append(pk)
    n = res["peaks"]["modal_n"]
    if (n < 2 or len(set(res["call"]))) == 1 and res.get("assign_method", "dist") == "dist":
        rcs = np.array(cns, dtype=int)
        rng.shuffle(rcs)
        part = rcs.shape[0] // 2
        return tuple(rcs[:part].tolist()), tuple(rcs[part:].tolist())
    rc = [[] for _ in range(n)]
    for cn, pk in zip(cns, peaks):
        rc[pk].append(cn)
    return tuple(map(tuple, rc))


def load_trio_json(path: str, seed: int = DEFAULT_SEED) -> TrioMember:
    """A `call --call-alleles` JSON report of this project (a report written by STRkit itself has the same keys)."""
    with open(path) as fh:
        report = json.load(fh)
    m = TrioMember()
    m.contigs = set(report["contigs"]) if report.get("contigs") is not None else {r["contig"] for r in report["results"]}
    for ordinal, res in enumerate(report["results"]):
        key = (res["contig"], int(res["start"]), int(res["end"]), res["motif"])
        if res.get("call") is None:
            m.loci[key] = None
            continue
        m.loci[key] = {"call": tuple(int(c) for c in res["call"]), "cis": tuple((int(lo), int(hi)) for lo, hi in res["call_95_cis"]),
                       "reads": split_reads_json(res, np.random.default_rng([int(seed), ordinal])), "ref_cn": int(res["ref_cn"]),
                       "seqs": None, "ps": res.get("ps") is not None}
    return m


def _vcf_lines(path: str):
    with open(path, "rb") as fh:
        gz = fh.read(2) == b"\x1f\x8b"
    with (gzip.open(path, "rt") if gz else open(path, "rt")) as fh:      # (as frontend/snv_vcf.py reads its VCF: no index)
        for line in fh:
            if line and line[0] != "#":
                yield line.rstrip("\r\n").split("\t")


def load_trio_vcf(path: str) -> TrioMember:
    """A VCF written by this project's `call` (plain or gzip), first sample."""
    m = TrioMember(has_seqs=True)
    for f in _vcf_lines(path):
        if len(f) < 10:
            continue
        info = dict(kv.split("=", 1) for kv in f[7].split(";") if "=" in kv)
        if info.get("VT") != "str":
            continue
        m.contigs.add(f[0])
        key = (f[0], int(info["BED_START"]), int(info["BED_END"]), info["MOTIF"])
        s = dict(zip(f[8].split(":"), f[9].split(":")))
        mc = s.get("MC", ".")
        if mc == "." or "." in mc.split(",") or s.get("MCCI", ".") == ".":
            m.loci[key] = None
            continue
        reads = ()
        if s.get("MCRL", ".") != ".":
            groups = [tuple(int(cn) for cn, c in (x.split("x") for x in g.split("|") if x) for _ in range(int(c))) for g in s["MCRL"].split(",")]
            reads = (groups[0][::2], groups[0][1::2]) if len(groups) == 1 else tuple(groups)      # one peak: interleaved
        alleles = [f[3]] + f[4].split(",")
        gt = re.split(r"[/|]", s.get("GT", "."))
        seqs = None if "." in gt or alleles[1:] == ["."] and any(g != "0" for g in gt) else tuple(sorted((alleles[int(g)] for g in gt), key=len))
        m.loci[key] = {"call": tuple(int(c) for c in mc.split(",")), "cis": tuple(tuple(int(x) for x in ci.split("-")) for ci in s["MCCI"].split(",")),
                       "reads": reads, "ref_cn": int(info["REFMC"]), "seqs": seqs, "ps": "PS" in s}
    return m


@dataclass
class TrioArrays:
    keys: list              # (contig, start, end, motif) of every trio-called locus, contigs sorted, file order inside
    packed: dict            # what pack_loci gives for them
    loci: list              # the dicts that were packed (gt, ci95, seqs, reads, ref_cn)
    n_loci_seen: int
    seen_lengths: list
    n_loci_skipped_ploidy: int
    includes_seq: bool


def assemble_trio(child: TrioMember, mother: TrioMember, father: TrioMember, contigs=None, only_phased: bool = False) -> TrioArrays:
    """base.py:144-167 and the loops of strkit.py: the contigs all three files share, without the sex chromosomes; a locus is seen
    when the child has it, trio-called when all three have a call under exactly the same (contig, start, end, motif).  Exact
    keys are this project's rule (its files come from one catalog); a member whose call has not two alleles makes the locus
    skipped and counted, because the reference's rule is diploid only."""
    shared = (child.contigs & mother.contigs & father.contigs) - SEX_CHROMOSOMES
    if contigs:
        shared &= set(contigs)
    keys, loci, seen, skipped = [], [], set(), 0
    for contig in sorted(shared):
        for key, c in child.loci.items():
            if key[0] != contig:
                continue
            seen.add(key[:3])
            m, f = mother.loci.get(key), father.loci.get(key)
            if c is None or m is None or f is None:
                continue
            if only_phased and not (c["ps"] and m["ps"] and f["ps"]):
                continue
            if any(len(x["call"]) != 2 or len(x["cis"]) != 2 for x in (c, m, f)):
                skipped += 1
                continue
            members = (c, m, f)
            reads = [tuple(x["reads"][k]) if k < len(x["reads"]) else () for x in members for k in range(2)]
            seqs = None
            if all(x["seqs"] is not None and len(x["seqs"]) == 2 for x in members):
                seqs = [s for x in members for s in x["seqs"]]
            keys.append(key)
            loci.append({"gt": [g for x in members for g in x["call"]], "ci95": [ci for x in members for ci in x["cis"]],
                         "seqs": seqs, "reads": reads, "ref_cn": c["ref_cn"]})
    return TrioArrays(keys, pack_loci(loci), loci, len(seen), [k[2] - k[1] for k in seen], skipped, child.has_seqs)


# ---- across loci ---------------------------------------------------------------------------------------------------------------
def correct_for_multiple_testing(p, sig_level: float, method: str = "none"):
    """(rejected, adjusted p) in the caller's order, from the methods' published definitions as statsmodels' multipletests states
    them (the package is not a dependency: this part is unpinned).  Step-down methods take the running maximum
    over ascending p, step-up methods the running minimum from the largest p down; adjusted p is clipped at 1; a hypothesis is
    rejected iff its adjusted p <= sig_level, and with "none" iff p < sig_level, which is what the reference does."""
    if method in ("fdr_tsbh", "fdr_tsbky"):
        raise ValueError(f"--mt-corr {method}: the two-stage methods fdr_tsbh and fdr_tsbky are not supported")
    if method not in MT_METHODS:
        raise ValueError(f"unknown multiple-testing method {method!r}")
    p = np.asarray(p, np.float64)
    n = p.size
    if method == "none":
        return p < sig_level, p.copy()
    order = np.argsort(p, kind="stable")
    ps = p[order]
    down = np.arange(n, 0, -1, dtype=np.float64)          # n .. 1
    with np.errstate(divide="ignore", invalid="ignore"):
        if method == "bonferroni":
            adj = ps * n
        elif method == "sidak":
            adj = -np.expm1(n * np.log1p(-ps))
        elif method == "holm":
            adj = np.maximum.accumulate(ps * down)
        elif method == "holm-sidak":
            adj = np.maximum.accumulate(-np.expm1(down * np.log1p(-ps)))
        elif method == "simes-hochberg":
            adj = np.minimum.accumulate((ps * down)[::-1])[::-1]
        else:
            cm = np.sum(1.0 / np.arange(1, n + 1)) if method == "fdr_by" else 1.0
            adj = np.minimum.accumulate((ps * n * cm / np.arange(1, n + 1))[::-1])[::-1]
    adj = np.minimum(adj, 1.0)
    out = np.empty(n)
    out[order] = adj
    return out <= sig_level, out


def _contig_rank(contig: str):
    c = contig[3:] if contig.startswith("chr") else contig
    return (0, int(c), "") if c.isdigit() else (1, 0, c)


def mi_result(trio: TrioArrays, out: dict, *, test: str = "none", sig_level: float = 0.05, mt_corr: str = "none", mismatch_out_mi: str = "pm1",
              bin_width: int = 10) -> dict | None:
    """The rates (base.py:177-272), the histogram (result.py:830-898) and the output loci (result.py:669-698, 765-768) of a trio
    from the arrays mi_trio_batch returned.  None when no locus is trio-called."""
    n = len(trio.keys)
    if n == 0:
        log.warning("No common loci found")
        return None
    r = out["respects"]
    shown = {"strict": True, "pm1": True, "ci_95": True, "ci_99": False, "seq": trio.includes_seq, "sl": trio.includes_seq, "sl_pm1": trio.includes_seq}
    rates = {k: (float((r[:, i] == 1).sum()) / n if shown[k] else None) for i, k in enumerate(KINDS)}
    p_adj = np.full(n, np.nan)
    if test == "none":
        col = r[:, KINDS.index(mismatch_out_mi)]
        idx = sorted(np.nonzero(col == 0)[0].tolist(), key=lambda i: (_contig_rank(trio.keys[i][0]), trio.keys[i][1], trio.keys[i][3]))
    else:
        tested = np.nonzero(out["status"] == _lib.STRK_MI_TESTED)[0]
        rej, adj = correct_for_multiple_testing(out["p"][tested], sig_level, mt_corr)
        p_adj[tested[rej]] = adj[rej]
        keep = tested[rej]
        sort_by = p_adj[keep] if mt_corr != "none" else out["p"][keep]
        idx = keep[np.argsort(sort_by, kind="stable")].tolist()
    lengths = np.array([k[2] - k[1] for k in trio.keys], np.int64)
    bins = np.arange(0, int(lengths.max()) + bin_width, bin_width).tolist()
    totals = np.bincount([x // bin_width for x in trio.seen_lengths if x // bin_width < len(bins)], minlength=len(bins))
    which = lengths // bin_width
    hist = []
    names = ("mi", "mi_pm1", "mi_95", "mi_99", "mi_seq", "mi_sl", "mi_sl_pm1")
    for b, lo in enumerate(bins):
        rows = r[which == b]
        entry = {"bin": lo, "bin_count": int(rows.shape[0]), "bin_total": int(totals[b])}
        for i, name in enumerate(names):
            known = rows[:, i][rows[:, i] >= 0]
            entry[name] = float(known.mean()) if known.size else None
        hist.append(entry)
    return {"mi": rates, "n_loci_trio_called": n, "n_loci_total": trio.n_loci_seen, "n_loci_skipped_ploidy": trio.n_loci_skipped_ploidy,
            "test": test, "mt_corr": mt_corr, "hist": hist, "output_index": idx, "p_adj": p_adj}


def _locus_dict(trio: TrioArrays, out: dict, res: dict, i: int) -> dict:
    l, (contig, start, end, motif) = trio.loci[i], trio.keys[i]
    d = {"contig": contig, "start": start, "end": end, "motif": motif}
    for m, who in enumerate(("child", "mother", "father")):
        d[who + "_gt"] = list(l["gt"][2 * m:2 * m + 2])
        d[who + "_gt_95_ci"] = [list(ci) for ci in l["ci95"][2 * m:2 * m + 2]]
        d[who + "_read_counts"] = [list(g) for g in l["reads"][2 * m:2 * m + 2]]
    p = float(out["p"][i])
    if res["test"] != "none" and p == p and p:      # (result.py:518: only a p that is not 0)
        d["p"] = p
        d["mutation_from"] = FROM_NAMES[int(out["mutation_from"][i])]
        if res["p_adj"][i] == res["p_adj"][i] and res["p_adj"][i]:
            d["p_adj"] = float(res["p_adj"][i])
    return d


def report_object(trio: TrioArrays, out: dict, res: dict) -> dict:
    """The report of result.py:715-753, plus n_loci_skipped_ploidy."""
    n_seen = max(res["n_loci_total"], 1)

    def entry(v):
        if v is None:
            return None
        se = math.sqrt((v * (1 - v)) / n_seen)
        return {"val": v, "est_std_err": se, "est_95_ci": [v - 1.96 * se, v + 1.96 * se]}

    m = res["mi"]
    return {"mi": entry(m["strict"]), "mi_pm1": entry(m["pm1"]), "mi_95": entry(m["ci_95"]), "mi_99": entry(m["ci_99"]),
            "mi_seq": entry(m["seq"]), "mi_sl": entry(m["sl"]), "mi_sl_pm1": entry(m["sl_pm1"]),
            "n_loci_trio_called": res["n_loci_trio_called"], "n_loci_total": res["n_loci_total"],
            "n_loci_skipped_ploidy": res["n_loci_skipped_ploidy"], "test": res["test"], "hist": res["hist"],
            "significant_loci": [_locus_dict(trio, out, res, i) for i in res["output_index"]]}


def write_report_json(trio: TrioArrays, out: dict, res: dict, path: str) -> None:
    text = json.dumps(report_object(trio, out, res), indent=2)
    if path == "stdout":
        print(text)
    else:
        with open(path, "w") as fh:
            fh.write(text + "\n")


def _pair(gt) -> str:
    return "|".join(str(x) for x in gt)


def locus_tsv(trio: TrioArrays, out: dict, res: dict, sep: str = "\t") -> str:
    """The columns of result.py:770-798: the key, per member the genotype and its 95 % and (empty) 99 % intervals, the reference
    copy number, then p, adjusted p (with a correction) and mutation_from (with a test)."""
    rows = []
    for i in res["output_index"]:
        l, key = trio.loci[i], trio.keys[i]
        cols = [key[0], str(key[1]), str(key[2]), key[3]]
        for m in range(3):
            cols += [_pair(l["gt"][2 * m:2 * m + 2]), "|".join(f"{lo},{hi}" for lo, hi in l["ci95"][2 * m:2 * m + 2]), ""]
        cols.append(str(l["ref_cn"] or ""))
        if res["test"] != "none":
            cols.append(str(float(out["p"][i])))
            if res["mt_corr"] != "none":
                cols.append(str(float(res["p_adj"][i])))
            cols.append(FROM_NAMES[int(out["mutation_from"][i])])
        rows.append(sep.join(cols) + "\n")
    return "".join(rows)


def summary_text(res: dict, widen: float = 0.0) -> str:
    names = {"strict": "MI%", "pm1": "MI% (±1)", "ci_95": "MI% (95% CI" + ("" if widen < 0.00001 else f"; widened {widen * 100:.1f}%") + ")",
             "ci_99": "MI% (99% CI)", "seq": "MI% (seq)", "sl": "MI% (seqlen)", "sl_pm1": "MI% (seqlen±1)"}
    cols = [(names[k], res["mi"][k]) for k in KINDS if k in ("strict", "pm1") or res["mi"][k]]
    return "".join(h.ljust(14) for h, _ in cols) + "\n" + "".join(f"{v * 100:.2f}".ljust(14) for _, v in cols)


def histogram_text(res: dict, bin_width: int = 10) -> str:
    """result.py:900-919: the bins, their counts and the rates per bin as tab-separated lines."""
    hist = res["hist"]

    def means(key):
        return "\t".join(f"{b[key] * 100:.2f}" if b[key] else "-" for b in hist)

    lines = ["\t".join(f"{b['bin']}-{b['bin'] + bin_width - 1}" for b in hist), "\t".join(str(b["bin_count"]) for b in hist), means("mi"), means("mi_pm1")]
    lines += [means(k) for k in ("mi_95", "mi_99") if any(b[k] for b in hist)]
    return "\n".join(lines)


def run_mi(child: str, mother: str, father: str, *, caller: str = "strkit-json", widen: float = 0.0, contigs=None, test: str = "none",
           sig_level: float = 0.05, mt_corr: str = "none", mismatch_out_mi: str = "pm1", only_phased: bool = False, seed: int = DEFAULT_SEED,
           bin_width: int = 10, device: str = "gpu"):
    """Files in, (trio, per-locus arrays, result) out; result is None when no locus is trio-called."""
    if mt_corr in ("fdr_tsbh", "fdr_tsbky") or mt_corr not in MT_METHODS:
        correct_for_multiple_testing([], sig_level, mt_corr)      # raises, naming the method
    if caller == "strkit-json":
        members = [load_trio_json(p, seed) for p in (child, mother, father)]
    elif caller == "strkit-vcf":
        members = [load_trio_vcf(p) for p in (child, mother, father)]
    else:
        raise ValueError(f"--caller {caller}: only strkit-json and strkit-vcf are supported")
    trio = assemble_trio(*members, contigs=contigs, only_phased=only_phased and caller == "strkit-vcf")
    if not trio.keys:
        return trio, None, mi_result(trio, {}, test=test)
    pk = trio.packed
    out = mi_trio_batch(pk["gt"], pk["ci95"], pk["grp_off"], pk["cn"], pk["ci99"], pk["seq_id"], pk["seq_len"], test=test,
                        sig_level=sig_level, widen=widen, device=device)
    if test != "none":
        for i in np.nonzero(out["status"] == _lib.STRK_MI_EMPTY_PARENT)[0]:
            contig, start, end, _ = trio.keys[i]
            reads = trio.loci[i]["reads"]
            first = next(c for c in CONFIGS if not reads[2 + c[0]] or not reads[4 + c[1]])
            who = [w for w, g in (("maternal", reads[2 + first[0]]), ("paternal", reads[4 + first[1]])) if not g]
            log.warning("%s:%d-%d - encountered empty readset for %s allele", contig, start, end, " and ".join(who))
    return trio, out, mi_result(trio, out, test=test, sig_level=sig_level, mt_corr=mt_corr, mismatch_out_mi=mismatch_out_mi, bin_width=bin_width)
