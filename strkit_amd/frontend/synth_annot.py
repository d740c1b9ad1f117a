"""Synthetic annotation files for `--gff`: a GFF3 and a GTF over the loci of a data set (synth_dataset.make_dataset, or any list of
loci), written as BGZF with their tabix index through synth_snvs' writers.  Test / benchmark input only; the index is generic
format 0 with columns 1 / 4 / 5, unpinned against htslib.  Contents: per contig one contig-long `region` as the
first line (NCBI's habit: it pulls every linear-index window back to the contig's start), nested genes / transcripts / exons / CDS
around a share of the loci, features between the loci, and contigs without features."""
from __future__ import annotations

import os

import numpy as np

from .synth_snvs import write_bgzf_vcf, write_tbi

__all__ = ["annotation_text", "index_annotations", "make_annotations"]


def _attrs(gtf: bool, pairs: list[tuple[str, str]]) -> str:
    if gtf:
        return " ".join(f'{k} "{v}";' for k, v in pairs)
    return ";".join(f"{k}={v}" for k, v in pairs)


def annotation_text(loci, contig_lengths: dict[str, int], gtf: bool = False, seed: int = 11, gene_share: float = 0.7,
                    between: int = 2, header: bool = True) -> bytes:
    """`loci`: (contig, start, end) triples.  Contigs of contig_lengths without loci get a region line only when their name ends in
    "_features"; others stay without features."""
    rng = np.random.default_rng(seed)
    by_contig: dict[str, list[tuple[int, int]]] = {c: [] for c in contig_lengths}
    for c, s, e in loci:
        by_contig.setdefault(c, []).append((int(s), int(e)))
    lines = ["##gff-version 3"] if header and not gtf else (["#!genome-build synthetic"] if header else [])
    n = 0
    for contig, length in contig_lengths.items():
        own = sorted(by_contig.get(contig, []))
        if not own and not contig.endswith("_features"):
            continue
        rows: list[tuple[int, int, str]] = []      # (start, order, line)

        def add(type_, start, end, pairs, strand="+"):
            start, end = max(1, int(start)), min(length, max(int(start), int(end)))
            rows.append((start, len(rows), f"{contig}\tsynth\t{type_}\t{start}\t{end}\t.\t{strand}\t.\t{_attrs(gtf, pairs)}"))

        add("region", 1, length, [("region_name", contig)] if gtf else [("ID", f"{contig}:1..{length}"), ("Dbxref", "taxon:9606"), ("Name", contig)])
        prev_end = 0
        for s, e in own:
            n += 1
            for _ in range(between):            # features between the loci: they overlap nothing, or only touch
                if s - prev_end > 400:
                    a = int(rng.integers(prev_end + 100, s - 200))
                    add("enhancer", a, min(a + int(rng.integers(10, 150)), s), [("enhancer_id", f"enh{n}.{a}")] if gtf else [("ID", f"enh{n}.{a}")])
            if rng.random() < gene_share:
                g0, g1 = s - int(rng.integers(50, 3000)), e + int(rng.integers(50, 3000))
                gene = [("gene_id", f"G{n}"), ("gene_name", f"STR{n}")] if gtf else [("ID", f"gene{n}"), ("Name", f"STR{n}"), ("biotype", "protein_coding")]
                add("gene", g0, g1, gene)
                for t in range(int(rng.integers(1, 3))):
                    tr = ([("gene_id", f"G{n}"), ("transcript_id", f"T{n}.{t}")] if gtf else [("ID", f"rna{n}.{t}"), ("Parent", f"gene{n}")])
                    add("transcript" if gtf else "mRNA", g0 + 10 * t, g1 - 10 * t, tr)
                    # one exon in front of the locus, one over it, one that only touches it (ends at s: start = s + 1 is past it)
                    for x, (a, b) in enumerate(((g0 + 10 * t, s - 20), (s - 5 + t, e + 7), (e + 1, g1 - 10 * t))):
                        if b < a:
                            continue
                        parent = [("gene_id", f"G{n}"), ("transcript_id", f"T{n}.{t}"), ("exon_number", str(x + 1))] if gtf else [("Parent", f"rna{n}.{t}")]
                        ex = parent + ([("exon_id", f"E{n}.{t}.{x}")] if (gtf or x % 2) else [])
                        add("exon", a + 1, b, ex if gtf or x != 1 else [("ID", f"exon{n}.{t}.{x}")] + ex)
                        if x == 1:
                            add("CDS", a + 2, b - 1, ex if t == 0 else parent)
                            add("start_codon", a + 2, a + 4, ex)
            prev_end = e
        rows.sort(key=lambda r: (r[0], r[1]))
        lines += [r[2] for r in rows]
    return ("\n".join(lines) + "\n").encode()


def index_annotations(text: bytes, gz_path: str, block_bytes: int = 0xFF00) -> str:
    """`text` as BGZF at gz_path with gz_path + ".tbi" next to it; returns gz_path."""
    offs = write_bgzf_vcf(gz_path, text, block_bytes)
    write_tbi(gz_path + ".tbi", text, offs, block_bytes, gff=True)
    return gz_path


def make_annotations(out_dir: str, loci, contig_lengths: dict[str, int], seed: int = 11, block_bytes: int = 0xFF00) -> dict:
    """genes.gff3.gz and genes.gtf.gz (with .tbi) under out_dir over `loci` ((contig, start, end) triples, or the truth records
    of synth_dataset.make_dataset, which lie on chr1) -> {"gff3": path, "gtf": path}."""
    loci = [("chr1", l["start"], l["end"]) if isinstance(l, dict) else tuple(l) for l in loci]
    os.makedirs(out_dir, exist_ok=True)
    out = {}
    for kind, gtf in (("gff3", False), ("gtf", True)):
        text = annotation_text(loci, contig_lengths, gtf=gtf, seed=seed)
        out[kind] = index_annotations(text, os.path.join(out_dir, f"genes.{kind}.gz"), block_bytes)
    return out
