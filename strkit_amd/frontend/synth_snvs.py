"""Synthetic SNV catalogs: a BGZF writer with blocks as small as asked for (so that lines straddle them), a tabix index writer
and a dbSNP-like VCF.  Test / benchmark input only.  Writer (here) and reader (`tabix.TabixIndex`) come from one reading of
the tabix specification: unpinned against htslib."""
from __future__ import annotations

import gzip
import struct
import zlib

import numpy as np

from .synth_large import _BGZF_EOF, _reg2bin

__all__ = ["write_bgzf_vcf", "write_tbi", "index_snv_vcf", "make_dbsnp_like"]


def _block(chunk: bytes, level: int = 1) -> bytes:
    comp = zlib.compressobj(level, zlib.DEFLATED, -15)
    body = comp.compress(chunk) + comp.flush()
    return (struct.pack("<BBBBIBBHBBHH", 0x1F, 0x8B, 8, 4, 0, 0, 0xFF, 6, 66, 67, 2, len(body) + 25) + body
            + struct.pack("<II", zlib.crc32(chunk), len(chunk)))


def write_bgzf_vcf(path: str, text: bytes, block_bytes: int = 0xFF00) -> np.ndarray:
    """`text` as BGZF blocks of `block_bytes` decompressed bytes each (the last one shorter) plus the EOF block; returns the
    compressed offset of every data block, then that of the EOF block."""
    assert 0 < block_bytes <= 0xFF00
    out = bytearray()
    offs = []
    for i in range(0, len(text), block_bytes):
        offs.append(len(out))
        out += _block(text[i:i + block_bytes])
    offs.append(len(out))
    out += _BGZF_EOF
    with open(path, "wb") as fh:
        fh.write(out)
    return np.array(offs, np.int64)


def _voff(block_off: np.ndarray, block_bytes: int, u: int) -> int:
    """Virtual offset of byte `u` of the text (the start of the next block rather than the end of one)."""
    return (int(block_off[u // block_bytes]) << 16) | (u % block_bytes)


def write_tbi(path: str, text: bytes, block_off: np.ndarray, block_bytes: int = 0xFF00, gff: bool = False) -> None:
    """The tabix index of the VCF `text` written by write_bgzf_vcf (coordinate-sorted within each contig, contigs in blocks).
    Every data line is a record of [POS - 1, POS - 1 + len(REF)); consecutive records of a bin share a chunk; linear windows no
    record overlaps take the preceding window's entry, as htslib fills them.  `gff`: the text is GFF3 / GTF instead: a data line is
    a record of [start - 1, end) (columns 4 and 5), in the bin of that extent and in the linear index of every window it overlaps,
    and the header says generic format 0 with columns 1 / 4 / 5 (`tabix -p gff`)."""
    names: list[bytes] = []
    bins: list[dict[int, list]] = []
    lin: list[dict[int, int]] = []
    u = 0
    for raw in text.split(b"\n"):
        a, u = u, u + len(raw) + 1
        f = raw.split(b"\t")
        if not raw or raw[:1] == b"#" or len(f) < (5 if gff else 4):
            continue
        try:
            pos0 = int(f[3 if gff else 1]) - 1
            end_gff = int(f[4]) if gff else 0
        except ValueError:
            pos0 = -1
        if not 0 <= pos0 < (1 << 29):      # what the index cannot place is left out of it (the bins end at 2^29)
            continue
        if f[0] not in names:
            names.append(f[0])
            bins.append({})
            lin.append({})
        t = names.index(f[0])
        end0 = min(max(end_gff, pos0 + 1), 1 << 29) if gff else pos0 + max(1, len(f[3].rstrip(b"\r")))
        v0, v1 = _voff(block_off, block_bytes, a), _voff(block_off, block_bytes, min(u, len(text)))
        ch = bins[t].setdefault(_reg2bin(pos0, end0), [])
        if ch and ch[-1][1] == v0:
            ch[-1][1] = v1
        else:
            ch.append([v0, v1])
        for w in range(pos0 >> 14, ((end0 - 1) >> 14) + 1):
            if w not in lin[t] or v0 < lin[t][w]:
                lin[t][w] = v0
    nm = b"".join(n + b"\0" for n in names)
    out = bytearray(b"TBI\x01" + struct.pack("<8i", len(names), 0 if gff else 2, 1, 4 if gff else 2, 5 if gff else 0, ord("#"), 0, len(nm)) + nm)
    for t in range(len(names)):
        out += struct.pack("<i", len(bins[t]))
        for b in sorted(bins[t]):
            out += struct.pack("<Ii", b, len(bins[t][b]))
            for c0, c1 in bins[t][b]:
                out += struct.pack("<QQ", c0, c1)
        n_win = max(lin[t]) + 1 if lin[t] else 0
        arr = np.zeros(n_win, np.uint64)
        for w, v in lin[t].items():
            arr[w] = v
        for w in range(1, n_win):
            if arr[w] == 0:
                arr[w] = arr[w - 1]
        out += struct.pack("<i", n_win) + arr.astype("<u8").tobytes()
    comp = bytearray()
    for i in range(0, len(out), 0xFF00):
        comp += _block(bytes(out[i:i + 0xFF00]), 6)
    with open(path, "wb") as fh:
        fh.write(comp + _BGZF_EOF)


def index_snv_vcf(plain_path: str, gz_path: str | None = None, block_bytes: int = 0xFF00) -> str:
    """<plain>.gz (BGZF) and <plain>.gz.tbi of a plain or gzip-compressed VCF; returns the .gz path."""
    with open(plain_path, "rb") as fh:
        text = fh.read()
    if text[:2] == b"\x1f\x8b":
        text = gzip.decompress(text)
    gz_path = gz_path or plain_path + ".gz"
    offs = write_bgzf_vcf(gz_path, text, block_bytes)
    write_tbi(gz_path + ".tbi", text, offs, block_bytes)
    return gz_path


def make_dbsnp_like(path: str, n_records: int, contig: str = "chr1", first: int = 1000, step: int = 97, seed: int = 1,
                    indel_share: float = 0.08, multi_share: float = 0.05) -> bytes:
    """A plain VCF of n_records lines on one contig, `step` bases apart on average: single-base records with rs ids and INFO
    fields of dbSNP's lengths (100 - 400 bytes), plus a share of indels and of multi-allelic lines.  Returns the text too."""
    rng = np.random.default_rng(seed)
    pos = first + np.cumsum(rng.integers(1, 2 * step, size=n_records))
    kind = rng.random(n_records)
    bases = "ACGT"
    ref_i = rng.integers(4, size=n_records)
    alt_i = (ref_i + 1 + rng.integers(3, size=n_records)) % 4
    info_len = rng.integers(100, 400, size=n_records)
    rs = rng.integers(1, 2_000_000_000, size=n_records)
    filler = ("RS=0;dbSNPBuildID=151;SSR=0;GENEINFO=LOC105378947:105378947;VC=SNV;GNO;FREQ=1000Genomes:0.9,0.1|GnomAD:0.95,0.05;" * 5)
    lines = ["##fileformat=VCFv4.2", f"##contig=<ID={contig}>", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"]
    for i in range(n_records):
        r = bases[ref_i[i]]
        if kind[i] < indel_share:
            ref, alt = r + bases[alt_i[i]] * 2, r
        elif kind[i] < indel_share + multi_share:
            ref, alt = r, bases[alt_i[i]] + "," + bases[(ref_i[i] + 2) % 4] + ("T" if kind[i] < indel_share + multi_share / 2 else "")
        else:
            ref, alt = r, bases[alt_i[i]]
        lines.append(f"{contig}\t{pos[i]}\trs{rs[i]}\t{ref}\t{alt}\t.\t.\t{filler[:info_len[i]]}")
    text = ("\n".join(lines) + "\n").encode()
    with open(path, "wb") as fh:
        fh.write(text)
    return text
