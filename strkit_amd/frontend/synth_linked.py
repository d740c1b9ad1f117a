"""Synthetic data for phase sets across loci: two contigs of diploid loci whose reads share heterozygous
sites with the reads of their neighbours, so that the SNV calls of neighbouring loci can be fitted into one phase set.  Every
read is cut out of one of two haplotypes that are consistent along the whole contig (a read that spans a second locus carries
that locus's allele of its haplotype too).  synth_phased.make_phased_dataset and its random stream are untouched; this
generator has a stream of its own."""
from __future__ import annotations

import os

import numpy as np

from .bam import write_bam
from .fasta import write_fasta
from .synth_dataset import _motif, _rand
from .synth_phased import _OTHER, _int_tag

__all__ = ["make_linked_dataset", "REGIONS"]

REGIONS = ("chain", "conflict", "bridge", "equal")


class _Contig:
    # the reference of one contig, built left to right: gaps, heterozygous sites inside gaps, loci
    def __init__(self, rng, name: str):
        self.rng, self.name = rng, name
        self.pieces: list[str] = []
        self.pos = 0
        self.loci: list[dict] = []
        self.sites: dict[str, int] = {}
        self._not_first = ""          # what the next gap must not begin with (the first base of the motif in front of it)

    def gap(self, n: int) -> None:
        s = _rand(self.rng, n)
        if self._not_first and s[0] == self._not_first:
            s = "ACGT".replace(self._not_first, "")[int(self.rng.integers(3))] + s[1:]
        self._not_first = ""
        self.pieces.append(s)
        self.pos += n

    def site(self, key: str) -> None:
        """The next base of the next gap is a heterozygous site."""
        self.sites[key] = self.pos

    def locus(self, locus_id: str, region: str, alleles: tuple[int, int], reach: tuple[int, int, int, int], override=None) -> dict:
        motif = _motif(self.rng, 3, 6)
        ref_cn = int(self.rng.integers(12, 24))
        if self.pieces[-1].endswith(motif[-1]):
            self.pieces[-1] = self.pieces[-1][:-1] + "ACGT".replace(motif[-1], "")[int(self.rng.integers(3))]
        L = {"id": locus_id, "region": region, "contig": self.name, "start": self.pos, "end": self.pos + ref_cn * len(motif), "motif": motif,
             "ref_cn": ref_cn, "alleles": (ref_cn + alleles[0], ref_cn + alleles[1]), "reach": reach, "override": override or {}}
        self.pieces.append(motif * ref_cn)
        self.pos = L["end"]
        self._not_first = motif[0]
        self.loci.append(L)
        return L


def _chain(c: _Contig, region: str, equal: bool) -> None:
    # 5 loci, a site in the middle of every gap and one beyond either end: the reads of a locus cover the site on either side of
    # it and nothing of the next locus.  The haplotype with the larger allele alternates from locus to locus.
    c.gap(1250)
    for i in range(5):
        c.site(f"{region}_g{i}")
        c.gap(750)
        d = (0, 0) if equal else ((-2, 4) if i % 2 else (4, -2))
        c.locus(f"{region}{i}", region, d, (900, 1100, 900, 1100))
        c.gap(750)
    c.site(f"{region}_g5")
    c.gap(1250)


def _bridge(c: _Contig) -> None:
    # A's reads reach s1 only, B's short reads s2 only; C's long reads reach both (and span B, where they are too few to make s1
    # useful): A and B open a phase set each, C joins the two
    c.gap(1500)
    c.locus("bridgeA", "bridge", (-3, 3), (800, 900, 600, 800))
    c.gap(500)
    c.site("bridge_s1")
    c.gap(700)
    c.locus("bridgeB", "bridge", (3, -2), (350, 450, 600, 800))
    c.gap(500)
    c.site("bridge_s2")
    c.gap(700)
    far = c.pos - c.sites["bridge_s1"]      # (A ends 500 in front of s1: 300 past s1 stays clear of A's flank)
    c.locus("bridgeC", "bridge", (-2, 4), (far + 100, far + 300, 800, 900))
    c.gap(1500)


def _conflict(c: _Contig) -> None:
    # A and B have reads of their own that cover one site; B's haplotype-1 reads carry a third base there
    c.gap(1500)
    c.locus("conflictA", "conflict", (-3, 2), (800, 900, 600, 800))
    c.gap(500)
    c.site("conflict_s")
    c.gap(700)
    c.locus("conflictB", "conflict", (3, -3), (800, 900, 800, 900), override={1: "conflict_s"})
    c.gap(1500)


def _cut_read(genome: str, hap: list[str], loci: list[dict], h: int, rs: int, re: int, override: dict[int, str]):
    """The read of haplotype `h` over the reference interval [rs, re): (sequence, CIGAR runs).  Every locus it touches lies
    inside it; `override`: position -> base, for this read alone."""
    seq, ops, pos = [], [], rs

    def gap(a, b):
        piece = hap[a:b]
        for p, base in override.items():
            if a <= p < b:
                piece = piece[:p - a] + [base] + piece[p - a + 1:]
        seq.append("".join(piece))
        ops.append((b - a, "M"))

    for L in loci:
        if L["end"] <= rs or L["start"] >= re:
            continue
        assert rs + 150 <= L["start"] and L["end"] + 150 <= re, (L["id"], rs, re)
        gap(pos, L["start"])
        k, cn = len(L["motif"]), L["alleles"][h]
        d = cn - L["ref_cn"]
        seq.append(L["motif"] * cn)
        ops += ([(L["ref_cn"] * k, "M")] + ([(d * k, "I")] if d else [])) if d >= 0 else [(cn * k, "M"), (-d * k, "D")]
        pos = L["end"]
    gap(pos, re)
    merged: list[tuple[int, str]] = []
    for n, op in ops:
        if merged and merged[-1][1] == op:
            merged[-1] = (merged[-1][0] + n, op)
        else:
            merged.append((n, op))
    return "".join(seq), merged


def make_linked_dataset(out_dir: str, reads_per_locus: int = 24, seed: int = 7, tags: str | None = None) -> dict:
    """Writes ref.fa, loci.bed, reads.bam and snvs.vcf under out_dir.  chr1 holds the regions `chain` (5 loci of unequal copy
    numbers, the haplotype with the larger allele alternating; neighbours' reads share the site between them), `conflict` (loci
    A < B with reads of their own over one site, where B's haplotype-1 reads carry a third base) and `bridge` (A < B < C: A's
    reads reach site s1 only, B's s2 only, C's both); chr2 holds `equal`, the chain's layout with equal copy numbers.  Haplotype
    0 is the reference outside the tracts, haplotype 1 carries the ALT base at every site; reads alternate between the two and
    are error-free.  `tags`: the reads of that one region carry HP = haplotype + 1 and one PS value.  Returns paths and the
    truth: `loci` (id, region, contig, start, end, alleles per haplotype, `het` = the sites its own reads cover) in catalog
    order, `sites` per contig, and per read name its haplotype."""
    rng = np.random.default_rng(seed)
    os.makedirs(out_dir, exist_ok=True)
    c1, c2 = _Contig(rng, "chr1"), _Contig(rng, "chr2")
    _chain(c1, "chain", equal=False)
    _conflict(c1)
    _bridge(c1)
    _chain(c2, "equal", equal=True)
    genomes, records, vcf, truth, read_hap = {}, [], [], [], {}
    for c in (c1, c2):
        genome = "".join(c.pieces)
        genomes[c.name] = genome
        haps = [list(genome), list(genome)]
        for key, p in c.sites.items():
            haps[1][p] = _OTHER[genome[p]]
            vcf.append((c.name, p, key, genome[p], _OTHER[genome[p]]))
        for L in c.loci:
            third = {p: next(b for b in "ACGT" if b not in (genome[p], _OTHER[genome[p]])) for p in (c.sites[k] for k in L["override"].values())}
            lo = hi = None
            for ri in range(reads_per_locus):
                h = ri % 2
                rs = L["start"] - int(rng.integers(L["reach"][0], L["reach"][1] + 1))
                re = L["end"] + int(rng.integers(L["reach"][2], L["reach"][3] + 1))
                lo, hi = rs if lo is None else max(lo, rs), re if hi is None else min(hi, re)
                seq, ops = _cut_read(genome, haps[h], c.loci, h, rs, re, third if h in L["override"] else {})
                name = f"{L['id']}_r{ri}"
                aux = b""
                if tags == L["region"]:
                    aux = _int_tag(b"HP", "C", h + 1) + _int_tag(b"PS", "i", 770000 + REGIONS.index(tags))
                records.append({"name": name, "flag": 0 if ri % 3 else 16, "contig": c.name, "pos": rs, "mapq": 60, "cigar": ops, "seq": seq,
                                "qual": np.full(len(seq), 40, np.uint8), "tags": aux})
                read_hap[name] = h
            truth.append({"id": L["id"], "region": L["region"], "contig": c.name, "start": L["start"], "end": L["end"], "alleles": L["alleles"],
                          "het": sorted(p for p in c.sites.values() if lo <= p < hi)})
    order = {"chr1": 0, "chr2": 1}
    records.sort(key=lambda r: (order[r["contig"]], r["pos"]))
    write_fasta(os.path.join(out_dir, "ref.fa"), genomes)
    with open(os.path.join(out_dir, "loci.bed"), "w") as fh:
        for c in (c1, c2):
            for L in c.loci:
                fh.write(f"{c.name}\t{L['start']}\t{L['end']}\tID={L['id']};MOTIF={L['motif']}\n")
    write_bam(os.path.join(out_dir, "reads.bam"), [(n, len(g)) for n, g in genomes.items()], records)
    with open(os.path.join(out_dir, "snvs.vcf"), "w") as fh:
        fh.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
        for contig, p, i, r, a in sorted(vcf):
            fh.write(f"{contig}\t{p + 1}\t{i}\t{r}\t{a}\t.\t.\t.\n")
    return {"paths": {k: os.path.join(out_dir, v) for k, v in (("ref", "ref.fa"), ("loci", "loci.bed"), ("bam", "reads.bam"), ("snvs", "snvs.vcf"))},
            "loci": truth, "sites": {c.name: dict(c.sites) for c in (c1, c2)}, "read_hap": read_hap}
