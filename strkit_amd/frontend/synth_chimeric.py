"""Synthetic data for read selection: synth_dataset.make_dataset's data set, and beside its clean alignment file
a second one with extra records: supplementary records (0x800, the name of a read of the locus, a hard-clipped partial
alignment over the locus) for a third of the loci, behind their primary in coordinate order for some reads and in front of it
for others, a few secondary records (0x100) under names of their own, and a few exact duplicates of a primary record.  One
long read spans two neighbouring loci and has a supplementary record over the second of them only: it is chimeric in that
region and not in the other (its primary is in both files).
make_dataset and its random stream are untouched; this generator has a stream of its own."""
from __future__ import annotations

import os

import numpy as np

from .bam import CIGAR_OPS, read_bam, write_bam
from .fasta import Fasta
from .synth_dataset import make_dataset

__all__ = ["make_chimeric_dataset"]


def _record(seg) -> dict:
    return dict(name=seg.name, flag=seg.flag, contig=seg.contig, pos=seg.start, mapq=seg.mapq,
                cigar=[(int(c) >> 4, CIGAR_OPS[int(c) & 15]) for c in seg.cigar], seq=seg.query_sequence, qual=seg.query_qualities)


def make_chimeric_dataset(out_dir: str, n_loci: int = 12, reads_per_locus: int = 12, seed: int = 7, extra_seed: int = 23, **dataset_keywords) -> dict:
    """make_dataset(out_dir, ...) and reads_chimeric.bam beside reads.bam.  Returns make_dataset's truth with
    paths["bam_clean"] (reads.bam), paths["bam"] (the file with the extra records) and `extras`:
    "supplementary": read name -> "after" | "before" (where its supplementary record lies relative to its primary; a record in
    front carries a tract two copies longer than the read's, so that it shows when it stands in for the read),
    "secondary": the names of the secondary records, "duplicates": the names of the duplicated primaries, "spanning": the long
    read {"name", "loci": the two loci (0-based) its primary spans, "chimeric_at": the one its supplementary record overlaps};
    with fewer than six loci there is none.  reads.bam is written again with the long read's primary in it."""
    ds = make_dataset(out_dir, n_loci=n_loci, reads_per_locus=reads_per_locus, seed=seed, **dataset_keywords)
    rng = np.random.default_rng(extra_seed)
    clean = read_bam(ds["paths"]["bam"])
    ref = Fasta(ds["paths"]["ref"])
    by_name = {s.name: s for s in clean.segments}
    records = [_record(s) for s in clean.segments]
    extras = {"supplementary": {}, "secondary": [], "duplicates": [], "spanning": None}
    clean_records = list(records)
    if len(ds["loci"]) >= 6:                              # a reference-allele read over loci 4 and 5, a supplementary record over 5
        a, b = ds["loci"][4], ds["loci"][5]
        contig = clean.contigs[0][0]

        def piece(beg, end, name, flag, clip):
            seq = ref.fetch(contig, beg, end)
            return dict(name=name, flag=flag, contig=contig, pos=beg, mapq=60, cigar=[(len(seq), "=")] + ([(clip, "H")] if clip else []),
                        seq=seq, qual=rng.integers(20, 41, size=len(seq)).astype(np.uint8))
        primary = piece(a["start"] - 300, b["end"] + 300, "span4_5", 0, 0)
        clean_records.append(primary)
        records += [primary, piece(b["start"] - 400, b["end"] + 280, "span4_5", 0x800, 900)]
        extras["spanning"] = {"name": "span4_5", "loci": (4, 5), "chimeric_at": 5}
    for li, L in enumerate(ds["loci"]):
        m, k = L["motif"], len(L["motif"])
        if li % 3 == 0:                                   # supplementary records for two reads of the locus, one each way
            for ri, where in ((0, "after"), (1, "before")):
                name = f"l{li}_r{ri}"
                seg = by_name.get(name)
                if seg is None:
                    continue
                r = _record(seg)
                flag = 0x800 | (seg.flag & 16)
                if where == "after":                      # the read without its first 50 bases
                    (n0, op0), rest = r["cigar"][0], r["cigar"][1:]
                    if op0 != "=" or n0 <= 60:
                        continue
                    records.append(dict(r, flag=flag, pos=seg.start + 50, cigar=[(50, "H"), (n0 - 50, op0)] + rest,
                                        seq=r["seq"][50:], qual=None if r["qual"] is None else r["qual"][50:]))
                else:                                     # 50 bases further left, a tract two copies longer, 300 bases of right flank
                    cn = L["reads"][name] + 2
                    left = ref.fetch(seg.contig, seg.start - 50, L["start"])
                    d = cn - L["ref_cn"]
                    cig = ([(len(left) + L["ref_cn"] * k, "=")] + ([(d * k, "I")] if d else []) if d >= 0
                           else [(len(left) + cn * k, "="), (-d * k, "D")])
                    read = left + m * cn + ref.fetch(seg.contig, L["end"], L["end"] + 300)
                    records.append(dict(r, flag=flag, pos=seg.start - 50, cigar=cig + [(300, "="), (max(1, seg.length - len(read)), "H")],
                                        seq=read, qual=rng.integers(20, 41, size=len(read)).astype(np.uint8)))
                extras["supplementary"][name] = where
        if li % 4 == 1:                                   # a secondary record under a name of its own: a copy of a read of the locus
            seg = by_name.get(f"l{li}_r2")
            if seg is not None:
                records.append(dict(_record(seg), name=f"sec{li}", flag=0x100 | (seg.flag & 16)))
                extras["secondary"].append(f"sec{li}")
        if li % 4 == 2:                                   # an exact duplicate of a primary record
            seg = by_name.get(f"l{li}_r3")
            if seg is not None:
                records.append(_record(seg))
                extras["duplicates"].append(seg.name)
    records.sort(key=lambda r: r["pos"])                  # (stable: a duplicate stays behind its original)
    if extras["spanning"]:
        clean_records.sort(key=lambda r: r["pos"])
        write_bam(ds["paths"]["bam"], clean.contigs, clean_records)
    path = os.path.join(out_dir, "reads_chimeric.bam")
    write_bam(path, clean.contigs, records)
    ds["paths"]["bam_clean"] = ds["paths"]["bam"]
    ds["paths"]["bam"] = path
    ds["extras"] = extras
    return ds
