"""What happens to the per-read copy numbers after the hot path: the records the reference's
allele calling starts from and the read-level fields of its VCF.

* `read_weights` — `locus_segments.get_read_weight(targeted, segment.length, tr_len_w_flank)` (call_locus.py:1259).  The
  Rust original is not in the reference's tree; the formula is the one STRkit's earlier pure-Python releases carried at
  this very spot, and it reproduces the documented example (docs/output_formats.md:92-104: `sl` 31, flank 70 -> `w`
  1.0217 for HiFi reads of ~15.8 kb).  UNPINNED like the rest of the un-vendored arithmetic.
* `allele_calling_inputs` — the two arrays `call_alleles_with_gmm` builds from the read records and hands to
  `allele.call_alleles` (call_locus.py:188-204; allele.py:176-189): int32 copy numbers, float64 weights normalised to 1.
* `mcrl_field` / `slr_field` — the `MCRL` / `SLR` sample fields (output/vcf.py:322-342): per allele ("peak") a histogram
  `CNxCOUNT|CNxCOUNT...` of the read-level copy numbers / tract lengths of the reads assigned to it.
* `write_vcf` — a VCF 4.2 text writer with the reference's header lines and the record layout of
  create_result_vcf_records (output/vcf.py:67-156,173-342) for what this backend knows.  A row with a `call` and allele
  sequences (`peaks.seqs`, call_sample(call_alleles=True, consensus=True)) gets `ALT`, `GT` and the per-allele fields as
  there (output/vcf.py:202-342); a row with a call and a `peaks` record but no sequences gets the per-allele counts and
  intervals and a blank `GT`; a row that carries peak labels (`p`) per read and a `call` only gets `MC` / `MCRL` / `SLR`
  per peak.  For rows without a call the reference writes none of the read-level fields; this writer adds, under its own
  header note, the one-group histograms of all kept reads so that the read-level answers of the hot path are visible in
  the VCF too.
"""
from __future__ import annotations

import os
from collections import Counter
from datetime import datetime

import numpy as np

from .genotype import n_alleles_of

__all__ = ["read_weights", "allele_calling_inputs", "format_count_pair", "mcrl_field", "slr_field", "write_vcf", "VCF_ANCHOR_SIZE"]

VCF_ANCHOR_SIZE = 5


def read_weights(read_lengths_sorted: np.ndarray, tr_len_with_flank: np.ndarray, read_length: np.ndarray | None = None,
                 targeted: bool = False) -> np.ndarray:
    """Weight of each read of ONE locus.  `read_lengths_sorted`: lengths of all segments fetched for the locus, ascending
    (`locus_segments.sorted_read_lengths`, call_locus.py:1057); `tr_len_with_flank` per read = |flank| + |tract| + |flank| as
    extracted (call_locus.py:1254).  A read large enough to contain the tract is the rarer the longer the tract is:
    w = (L + t - 2) / (L - t + 1) with L the mean length of the reads that could contain it (targeted: the read's own
    length).  NaN where no fetched read is long enough (the reference voids the locus there, call_locus.py:1261-1271)."""
    t = np.asarray(tr_len_with_flank, np.float64)
    lens = np.asarray(read_lengths_sorted, np.float64)
    if targeted:
        L = np.asarray(read_length, np.float64)
    else:
        part = np.searchsorted(lens, t, side="left")
        suffix = np.concatenate((np.cumsum(lens[::-1])[::-1], [0.0]))
        cnt = len(lens) - part
        L = np.where(cnt > 0, suffix[np.minimum(part, len(lens))] / np.maximum(cnt, 1), np.nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (L + t - 2.0) / (L - t + 1.0)


def block_read_weights(counts, item_locus, lens_all, read_locus, tlwf) -> np.ndarray:
    """read_weights for the kept reads of all loci of a block at once.  `counts`: records fetched per locus; `item_locus`,
    `lens_all`: locus and sequence length of every fetched record (ALL of them, sorted here inside the locus); `read_locus`,
    `tlwf`: locus and flank + tract + flank of every kept read.  L = mean length of the records that could contain it."""
    big = np.int64(1) << 40
    order = np.lexsort((lens_all, item_locus))
    key = item_locus[order] * big + lens_all[order]
    csum = np.concatenate(([0], np.cumsum(lens_all[order])))
    loc_end = np.cumsum(counts)                                   # end of each locus' run in `order`
    part = np.searchsorted(key, read_locus * big + tlwf, side="left")
    e_ = loc_end[read_locus]
    L = (csum[e_] - csum[part]) / np.maximum(e_ - part, 1)
    return (L + tlwf - 2.0) / (L - tlwf + 1.0)


def allele_calling_inputs(row: dict) -> tuple[np.ndarray, np.ndarray]:
    """(read_cns int32, read_weights float64 summing to 1) of a result row, in read order — exactly what
    call_alleles_with_gmm derives from `read_dict` (call_locus.py:188-192) and passes as `repeats_fwd` /
    `read_weights_fwd` to allele.call_alleles (call_locus.py:201-214)."""
    rdvs = tuple((row.get("reads") or {}).values())
    cns = np.fromiter((r["cn"] for r in rdvs), dtype=np.int32, count=len(rdvs))
    w = np.fromiter((r["w"] for r in rdvs), dtype=np.float64, count=len(rdvs))
    if len(w):
        w /= w.sum()
    return cns, w


def format_count_pair(pair) -> str:
    return "x".join(map(str, pair))      # CNxCOUNT or SLxCOUNT (output/vcf.py:57-58)


def _hist_field(reads: dict, key: str, n_peaks: int | None) -> tuple[str, ...]:
    vals = list(reads.values())
    if n_peaks is None:                  # no peak labels: one group with every read
        groups = [vals]
    else:
        groups = [[r for r in vals if r.get("p") == pi] for pi in range(n_peaks)]
    return tuple("|".join(map(format_count_pair, sorted(Counter(r[key] for r in g).items()))) for g in groups)


def mcrl_field(reads: dict, n_peaks: int | None = None) -> tuple[str, ...]:
    """`MCRL` (output/vcf.py:322-330): e.g. ("7x1|8x10|9x1", "8x2|9x12") for two alleles of 8 and 9 copies."""
    return _hist_field(reads, "cn", n_peaks)


def slr_field(reads: dict, n_peaks: int | None = None) -> tuple[str, ...]:
    """`SLR` (output/vcf.py:332-342): the same for the read-level tract lengths."""
    return _hist_field(reads, "sl", n_peaks)


_FORMATS = (("AD", ".", "Integer", "Read depth for each allele"),
            ("DP", "1", "Integer", "Read depth"),
            ("DPS", "1", "Integer", "Read depth (supporting reads only)"),
            ("GT", "1", "String", "Genotype"),
            ("MC", ".", "Integer", "Motif copy number for each allele"),
            ("MCCI", ".", "String", "Motif copy number 95% confidence interval for each allele"),
            ("MCRL", ".", "String", "Read-level motif copy numbers for each allele"),
            ("MMAS", "1", "Float", "Mean model (candidate TR sequence) alignment score across reads."),
            ("PM", "1", "String", "Peak-calling method (dist/snv+dist/snv/hp)"),
            ("SLR", ".", "String", "Read-level sequence lengths for each allele"))
_SEQ_FORMATS = (("ANCL", ".", "Integer", "Anchor length for the ref and each alt, five-prime of TR sequence"),
                ("CONS", ".", "String", "Consensus methods used for each alt (single/poa/best_rep)"))
_INFOS = (("VT", "1", "String", "Variant record type (str/snv)"),
          ("MOTIF", "1", "String", "Motif string"),
          ("REFMC", "1", "Integer", "Motif copy number in the reference genome"),
          ("BED_START", "1", "Integer", "Original start position of the locus as defined in the catalog (0-based inclusive)"),
          ("BED_END", "1", "Integer", "Original end position of the locus as defined in the catalog (0-based exclusive, i.e., 1-based)"),
          ("ANCH", "1", "Integer", "Five-prime anchor size"))


_INFO_ANNOT = ("ANNOT", "1", "String", "Locus annotations (e.g., genomic regions)")      # output/vcf.py:148


def _annot_value(ids) -> str:
    """The ids joined by ',' as the reference joins them (output/vcf.py:275), each with the characters an INFO value cannot hold
    percent-encoded (VCF 4.3 §1.2; '%' itself too, so that the encoding can be undone)."""
    enc = {"%": "%25", " ": "%20", ";": "%3B", "=": "%3D", ",": "%2C"}
    return ",".join("".join(enc.get(ch, ch) for ch in i) for i in ids)


def _has_seqs(row: dict) -> bool:
    return bool(row.get("call")) and bool((row.get("peaks") or {}).get("seqs"))


def _alleles_of_row(row: dict, anchor: str, ref_seq: str, n_alleles: int):
    """output/vcf.py:202-287 for a row with a call and allele sequences: (anchor offset, the alleles as (tract, anchor) pairs
    with the reference first and None for "no alternative", the VCF allele strings, the genotype indices, the method per
    distinct sequence), or None where the reference skips the record (a missing sequence, an allele it cannot index)."""
    peaks = row["peaks"]
    methods = {(seq.upper() if seq else seq): method for seq, method in peaks["seqs"]}
    peak_seqs = tuple(methods)
    anchors = [a for a, _ in peaks.get("start_anchor_seqs") or []]
    if any(s is None for s in peak_seqs) or any(a is None for a in anchors):
        return None
    anchors = tuple(a.upper() for a in anchors)
    # bases shared by the front of every anchor are cut; one base stays as the anchor VCF needs
    offset = min(len(os.path.commonprefix([anchor, *anchors])), VCF_ANCHOR_SIZE - 1, max(len(anchor) - 1, 0))
    ref_anchor = anchor[offset:]
    with_anchors = list(zip(peak_seqs, (a[offset:] for a in anchors)))
    if 0 < len(with_anchors) < n_alleles:
        with_anchors = [with_anchors[0]] * n_alleles
    alts = sorted({c for c in with_anchors if c[1] + c[0] != ref_anchor + ref_seq}, key=lambda c: c[1] + c[0])
    raw = ((ref_seq, ref_anchor), *(alts or (None,)))
    # a complete deletion, anchor included, is the symbolic "upstream deletion" allele
    strings = [ref_anchor + ref_seq] + (["*" if not t and not a else a + t for t, a in alts] if alts else ["."])
    try:
        gt = tuple(raw.index(c) for c in with_anchors)
    except ValueError:
        return None
    return offset, raw, strings, gt, methods


def write_vcf(report: dict, path: str, ref=None, sample_id: str | None = None, n_alleles: int | dict | None = None,
              date: str | None = None) -> int:
    """Writes the loci of a report as VCF 4.2 text; returns the number of records.  `ref` (a Fasta) supplies the contig
    lengths of the header.  Loci without reference data have no anchor and are skipped, as the reference does
    (output/vcf.py:184-186).  `n_alleles` (one number, or a dict per contig): the report's own when not given, else 2.  A
    report of a run with snv_phase_sets also gets the called SNVs of its rows as `VT=snv` records, sorted in by position."""
    if n_alleles is None:
        params = report.get("parameters") or {}
        n_alleles = params.get("n_alleles", 2)
        if params.get("ploidy") is not None:      # the run's ploidy configuration says how many alleles a contig has
            from ..ploidy import load_ploidy_config
            n_alleles = load_ploidy_config(params["ploidy"])
    formats = _FORMATS
    if any(_has_seqs(r) for r in report["results"]):
        formats = _FORMATS[:1] + _SEQ_FORMATS + _FORMATS[1:]
    # phased rows: the two fields are declared only when a row carries them, so that a report without them
    # gives the bytes it always gave
    extra = ([("NSNV", "1", "Integer", "Number of supporting SNVs for the STR peak-call")] if any(r.get("snvs") for r in report["results"]) else []) + \
            ([("PS", "1", "Integer", "Phase set")] if any(r.get("ps") is not None for r in report["results"]) else [])
    use_methyl = bool((report.get("parameters") or {}).get("use_methyl"))
    if use_methyl:      # (output/vcf.py:114-116: declared by the run's switch, not by what the rows carry)
        extra += [("AM", ".", "Float", "Average methylation level (5-methyl CpG sites) for each allele"),
                  ("AMC", ".", "Float", "Average number of 5-methyl CpG sites for each allele")]
    if extra:
        formats = tuple(sorted(formats + tuple(extra), key=lambda f: f[0]))
    sample = sample_id or report.get("sample_id") or "sample"
    now = datetime.now()  # noqa: DTZ005
    lines = ["##fileformat=VCFv4.2", "##fileDate=" + (date or f"{now.year}{now.month:02d}{now.day:02d}"), "##source=strkit_amd",
             "##strkitCommand=call", f"##strkitCatalogNumLoci={report.get('catalog', {}).get('num_loci', len(report['results']))}",
             "##strkitAmdNote=rows without an allele call carry MCRL and SLR as ONE group over all kept reads (STRkit writes them per called allele only)"]
    if ref is not None:
        lines += [f"##contig=<ID={c},length={ref.get_reference_length(c)}>" for c in ref.references]
    lines += [f'##FORMAT=<ID={i},Number={n},Type={t},Description="{d}">' for i, n, t, d in formats]
    annot = bool((report.get("parameters") or {}).get("annotation_file"))      # (--gff: ANNOT exists only in such a report's VCF)
    lines += [f'##INFO=<ID={i},Number={n},Type={t},Description="{d}">' for i, n, t, d in _INFOS + ((_INFO_ANNOT,) if annot else ())]
    lines.append("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + sample)
    n_rec = 0
    # snv_phase_sets: the only switch that changes what is written for a row's SNVs
    snv_records = bool((report.get("parameters") or {}).get("snv_phase_sets"))
    records: list[tuple] = []
    snvs_written: set = set()
    for row in sorted(report["results"], key=lambda r: (r["contig"], r.get("start_adj", r["start"]))):
        if "ref_start_anchor" not in row or "ref_seq" not in row:
            continue
        anchor, ref_seq = row["ref_start_anchor"].upper(), row["ref_seq"].upper()
        # without consensus sequences of the alleles nothing of the anchor is shared and can be cut: one base stays for VCF
        # compliance only when alleles are written; here the whole anchor is kept (anchor_offset 0, output/vcf.py:213-218)
        start0 = row.get("start_adj", row["start"]) - len(anchor)
        reads = row.get("reads") or {}
        call = row.get("call")
        n_peaks = len(call) if call else None
        n_al = n_alleles_of(n_alleles, row["contig"])
        peaks = (row.get("peaks") or None) if call else None      # per-allele fields are keyed on what the row carries
        alleles = None
        ref_allele, alt, gt = anchor + ref_seq, ".", "/".join(["."] * n_al)
        if peaks and peaks.get("seqs"):
            alleles = _alleles_of_row(row, anchor, ref_seq, n_al)
            if alleles is None:
                continue
            offset, raw, strings, gt_idx, methods = alleles
            anchor = anchor[offset:]
            start0 += offset
            ref_allele, alt, gt = strings[0], ",".join(strings[1:]), ("|" if row.get("ps") is not None else "/").join(map(str, gt_idx))
        if peaks:
            n_peaks = int(peaks["modal_n"])
        info = f"VT=str;MOTIF={row['motif']};REFMC={row['ref_cn']};BED_START={row['start']};BED_END={row['end']};ANCH={len(anchor)}"
        if annot and row.get("annotations"):
            info += ";ANNOT=" + _annot_value(row["annotations"])
        keys, vals = ["GT", "DP"], [gt, str(len(reads))]
        if row.get("assign_method"):
            keys.append("PM"); vals.append(str(row["assign_method"]))
        if call and row.get("snvs"):
            keys.append("NSNV"); vals.append(str(len(row["snvs"])))
        if call and row.get("ps") is not None:
            keys.append("PS"); vals.append(str(row["ps"]))
        if peaks:
            mmas = row.get("mean_model_align_score")
            keys += ["MMAS", "DPS", "AD"]
            # (a call of more than two peaks labels no read: no depth per allele)
            vals += ["." if mmas is None else f"{mmas:.6g}", str(sum(peaks["n_reads"])), ",".join(map(str, peaks["n_reads"])) or "."]
        if use_methyl and peaks:      # output/vcf.py:343-346: per allele, '.' per peak where the row has none
            for key in ("am", "amc"):
                keys.append(key.upper()); vals.append(",".join(f"{x:.6g}" for x in peaks[key]) if peaks.get(key) else ",".join(["."] * n_peaks))
        if call:
            keys.append("MC"); vals.append(",".join(str(int(c)) for c in call))
        if peaks:
            keys.append("MCCI"); vals.append(",".join(f"{lo}-{hi}" for lo, hi in row["call_95_cis"]))
        if alleles is not None:
            cons = [methods[ar[0]] for ar in raw[1:] if ar is not None]
            keys += ["ANCL", "CONS"]
            vals += [",".join(str(len(ar[1])) for ar in raw if ar is not None), ",".join(cons) if cons else "."]
        if reads:
            if n_peaks is not None and not row.get("read_peaks_called", True):
                n_peaks = None      # a call whose reads carry no peak: one group over all kept reads, as rows without a call
            keys += ["MCRL", "SLR"]
            vals += [",".join(mcrl_field(reads, n_peaks)), ",".join(slr_field(reads, n_peaks))]
        records.append((row["contig"], start0 + 1, 0, "\t".join((row["contig"], str(start0 + 1), row["locus_id"], ref_allele, alt, ".", ".", info,
                                                                  ":".join(keys), ":".join(vals)))))
        n_rec += 1
        if not snv_records or not call:
            continue
        # the row's called SNVs as records of their own (output/vcf.py:359-392), each once per contig, by the first row that holds it
        ps = row.get("ps")
        for snv in row.get("snvs") or []:
            if (row["contig"], snv["id"]) in snvs_written:
                continue
            snvs_written.add((row["contig"], snv["id"]))
            snv_alleles = (snv["ref"], *sorted({b for b in snv["call"] if b != snv["ref"]}))
            if len(snv_alleles) < 2:
                continue
            keys = ["GT", "DP", "AD"] + (["PS"] if ps is not None else [])
            vals = [("|" if ps is not None else "/").join(str(snv_alleles.index(b)) for b in snv["call"]), str(sum(snv["rcs"])),
                    ",".join(map(str, snv["rcs"]))] + ([str(ps)] if ps is not None else [])      # (AD in call order, as there)
            records.append((row["contig"], snv["pos"] + 1, 1, "\t".join((row["contig"], str(snv["pos"] + 1), snv["id"], snv_alleles[0],
                                                                          ",".join(snv_alleles[1:]), ".", ".", "VT=snv", ":".join(keys), ":".join(vals)))))
            n_rec += 1
    if snv_records:      # SNV records among the STR records by position; at one position the STR record comes first
        records.sort(key=lambda r: r[:3])
    lines += [r[3] for r in records]
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return n_rec
