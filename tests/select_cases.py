"""The corpus of the read-selection tests: one small BAM's worth of records (one-base to ten-base sequences, a `<n>M` CIGAR,
names as raw bytes) and loci as lists of record indices in file order, built from strk_select_constants() so that it follows
the kernels as built.  Shared by tests/test_select_rule.py (host, against the restatement) and tests/test_gpu_select.py."""
import functools
import struct
from dataclasses import dataclass, field

import numpy as np

from strkit_amd.frontend.bam import _bgzf_blocks
from strkit_amd.frontend.select import select_constants

NO_CAP = (1 << 31) - 1
SEED = 20261020


@dataclass
class Corpus:
    names: list = field(default_factory=list)        # bytes per record, file order
    flags: list = field(default_factory=list)
    loci: dict = field(default_factory=dict)         # case name -> record indices (ascending: file order)
    constants: dict = field(default_factory=dict)

    def add(self, name: bytes, flag: int = 0) -> int:
        self.names.append(bytes(name))
        self.flags.append(int(flag))
        return len(self.names) - 1

    def items(self, locus: str) -> list:
        return [(self.names[i], self.flags[i]) for i in self.loci[locus]]

    def bam_bytes(self) -> bytes:
        """The decompressed stream: header, then record i at position 10 * i of chr1."""
        rng = np.random.default_rng(SEED + 1)
        text = b"@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chr1\tLN:100000000\n"
        buf = bytearray(b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", 1))
        buf += struct.pack("<i", 5) + b"chr1\0" + struct.pack("<i", 100000000)
        for i, (name, flag) in enumerate(zip(self.names, self.flags)):
            l_seq = 1 + int(rng.integers(10))
            body = struct.pack("<iiBBHHHIiii", 0, 10 * i, len(name) + 1, 60, 4681, 1, flag, l_seq, -1, -1, 0)
            body += name + b"\0" + struct.pack("<I", l_seq << 4) + bytes(rng.integers(1, 16, size=(l_seq + 1) // 2).astype(np.uint8) * 17)
            body += bytes([30]) * l_seq
            buf += struct.pack("<i", len(body)) + body
        return bytes(buf)

    def write(self, path: str) -> str:
        with open(path, "wb") as fh:
            fh.write(_bgzf_blocks(self.bam_bytes()))
        return path

    def item_arrays(self, rec_off: np.ndarray, loci: list) -> tuple:
        """(item_off, rec_off per item) of the loci named, for the library's entry points."""
        idx = [np.asarray(self.loci[k], np.int64) for k in loci]
        item_off = np.concatenate(([0], np.cumsum([len(x) for x in idx]))).astype(np.int64)
        return item_off, np.ascontiguousarray(rec_off[np.concatenate(idx)] if idx and item_off[-1] else np.zeros(0, np.int64), np.int64)


FLAG_CHOICES = (0, 16, 0, 16, 0x100, 0x110, 0x800, 0x810, 0x900)


@functools.lru_cache(maxsize=None)
def corpus() -> Corpus:
    c = Corpus(constants=select_constants())
    cls, slots, step = c.constants["small_items"], c.constants["small_slots"], c.constants["compare_step"]
    rng = np.random.default_rng(SEED)
    # the pool: more distinct names than the small table has slots, of odd and even lengths (record offsets then take every
    # residue mod 4); every seventh has a twin right behind it, every third one far behind (after the whole pool)
    n_base = slots + 150
    seen, base, near = set(), [], {}
    while len(base) < n_base:
        name = bytes(rng.integers(1, 256, size=int(rng.integers(1, 31))).astype(np.uint8))
        if name in seen:
            continue
        seen.add(name)
        i = len(base)
        base.append(c.add(name, FLAG_CHOICES[int(rng.integers(len(FLAG_CHOICES)))]))
        if i % 7 == 0:
            near[i] = c.add(name, FLAG_CHOICES[int(rng.integers(len(FLAG_CHOICES)))])
    far = {i: c.add(c.names[base[i]], FLAG_CHOICES[int(rng.integers(len(FLAG_CHOICES)))]) for i in range(0, n_base, 3)}
    pool_end = len(c.names)
    in_order = list(range(base[0], far[0]))              # the pool's front part in file order (base records and near twins)

    def sized(n):                                          # n items: four fifths from the front part, the rest far twins of them
        a = in_order[:n - n // 5]
        have = set(a)
        b = [far[i] for i in sorted(far) if base[i] in have][:n // 5]
        a = in_order[:n - len(b)]
        return a + b

    for n in (0, 1, 2, 63, 64, 65, 255, 256, 257, cls - 1, cls, cls + 1):
        c.loci[f"size_{n}"] = sized(n)
    c.loci["large_many_names"] = list(range(pool_end))     # every record of the pool: more distinct names than the small table's slots
    # every name exactly twice, 300 items apart
    twice = [i for i in range(0, n_base, 3)][:300]
    c.loci["twice_far"] = [base[i] for i in twice] + [far[i] for i in twice]
    # all items share one name
    c.loci["one_name"] = [c.add(b"same", FLAG_CHOICES[k % len(FLAG_CHOICES)]) for k in range(130)]
    # name shapes
    shapes = [b"a", b"", bytes(range(1, 255)), bytes(range(2, 256)), bytes([7]) * 254,
              b"tail_x", b"tail_y", b"xhead", b"yhead", b"prefix", b"prefix_longer"]
    for n in (step - 1, step, step + 1, 2 * step, 2 * step + 1, 3 * step - 1):
        stem = bytes(65 + k for k in range(n))
        shapes += [stem, stem[:-1] + b"~", b"~" + stem[1:]] if n > 0 else [stem]
    shapes = list(dict.fromkeys(shapes))
    c.loci["shapes"] = [c.add(s, 0) for s in shapes] + [c.add(s, 0x800 if k % 2 else 0) for k, s in enumerate(shapes)]
    # flags
    def flags_locus(key, pairs):
        c.loci[key] = [c.add(n, f) for n, f in pairs]
    flags_locus("supp_only", [(b"X", 0x800)])
    flags_locus("primary_supp", [(b"A", 0), (b"A", 0x800)])
    flags_locus("supp_primary", [(b"B", 0x800), (b"B", 16)])
    flags_locus("primary_sec", [(b"C", 0), (b"C", 0x100)])
    flags_locus("sec_supp", [(b"D", 0x100), (b"D", 0x800)])
    flags_locus("sec_primary", [(b"F", 0x100), (b"F", 0)])
    flags_locus("both_bits", [(b"G", 0x900), (b"G", 0), (b"H", 0x900)])
    c.loci["flags_all"] = [i for k in ("supp_only", "primary_supp", "supp_primary", "primary_sec", "sec_supp", "sec_primary", "both_bits")
                           for i in c.loci[k]]
    return c


CAP_LOCUS = "size_257"


def caps(c: Corpus, rules: int) -> list:
    """max_reads values around the number of survivors of CAP_LOCUS under `rules`, and the two ends."""
    from select_restatement import survivors
    s = survivors(c.items(CAP_LOCUS), rules)
    return sorted({1, max(1, s - 1), s, s + 1, NO_CAP})


def expected(c: Corpus, loci: list, rules: int, max_reads: int) -> tuple:
    """(reason, status, n_kept) of the loci named, concatenated, by the restatement."""
    from select_restatement import select
    reason, status, kept = [], [], []
    for k in loci:
        r, s, n = select(c.items(k), rules, max_reads)
        reason += r
        status += s
        kept.append(n)
    return np.array(reason, np.uint8), np.array(status, np.uint8), np.array(kept, np.int32)
