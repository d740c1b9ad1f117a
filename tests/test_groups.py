"""strkit_amd/_groups.py on the CPU: packing lists of strings, and the arguments of the three *_packed calls (no library load)."""
import numpy as np
import pytest

from strkit_amd._groups import group_args, pack_groups

SHAPES = "group_off needs at least one entry, and seq_start and seq_len one entry per sequence"
SHAPES_K = "group_off needs at least one entry, seq_start and seq_len one entry per sequence, k one per group"


def _unpack(off, starts, lens, buf):
    text = buf.tobytes()
    return [[text[starts[i]:starts[i] + lens[i]] for i in range(off[g], off[g + 1])] for g in range(len(off) - 1)]


@pytest.mark.parametrize("groups", [
    [["CAG", "CAGCAG"], ["A"]],
    [[b"CAG", b"\x00\xff\x80"], [b"A"]],
    [["CAG", b"CAT"], [bytearray(b"AC"), np.frombuffer(b"GT", np.uint8)]],
    [[], ["CAG"], [], [], ["A", "C"], []],
    [["", "CAG", ""], [""], ["", ""]],
    [[]],
    [],
])
def test_pack_groups(groups):
    off, starts, lens, buf = pack_groups(groups)
    assert (off.dtype, starts.dtype, lens.dtype, buf.dtype) == (np.int32, np.int64, np.int32, np.uint8)
    want = [[s.encode("ascii") if isinstance(s, str) else bytes(s) for s in g] for g in groups]
    assert off.tolist() == [0] + np.cumsum([len(g) for g in want]).astype(int).tolist()
    assert lens.tolist() == [len(s) for g in want for s in g]
    assert starts.tolist() == np.concatenate(([0], np.cumsum(lens)))[:-1].tolist()
    assert buf.tobytes() == b"".join(s for g in want for s in g)
    assert _unpack(off.tolist(), starts.tolist(), lens.tolist(), buf) == want


def test_pack_groups_refuses_text_that_is_not_ascii():
    with pytest.raises(UnicodeEncodeError):
        pack_groups([["CAGé"]])


GOOD = ([0, 2, 3], [0, 3, 6], [3, 3, 2])


def _refused(text, off=GOOD[0], starts=GOOD[1], lens=GOOD[2], seqs=b"CAGCATAC", d_seqs=None, n=None, **kw):
    with pytest.raises(ValueError) as e:
        group_args(off, starts, lens, seqs, d_seqs, n, **kw)
    assert str(e.value) == text


def test_group_args_raises_what_the_packed_calls_raised():
    _refused(SHAPES, off=[])                                          # no entry in group_off
    _refused(SHAPES, starts=[0, 3])                                   # seq_start and seq_len of different shapes
    _refused(SHAPES, starts=[[0, 3, 6]], lens=[[3, 3, 2]])            # not one-dimensional
    _refused(SHAPES_K, off=[], shapes=SHAPES_K)                       # count_kmers_packed's wording
    _refused(SHAPES_K, starts=[0, 3], shapes=SHAPES_K)
    _refused("group_off must span seq_start / seq_len", off=[0, 2, 4])
    _refused("group_off must span seq_start / seq_len", off=[0, 2])
    _refused("exactly one of seqs (host) and d_seqs (device) must be given", seqs=None)
    _refused("exactly one of seqs (host) and d_seqs (device) must be given", d_seqs=4096, n=8)
    _refused("n_seq_bytes exceeds the buffer", n=9)
    _refused("d_seqs needs n_seq_bytes", seqs=None, d_seqs=4096)
    # the order of the checks, as it was: shapes, span, seqs xor d_seqs, the size
    _refused(SHAPES, off=[], seqs=None)
    _refused("group_off must span seq_start / seq_len", off=[0, 2], seqs=None)
    _refused("exactly one of seqs (host) and d_seqs (device) must be given", seqs=None, n=99)


@pytest.mark.parametrize("seqs", [b"CAGCATAC", bytearray(b"CAGCATAC"), memoryview(b"CAGCATAC"),
                                  np.frombuffer(b"CAGCATAC", np.uint8), list(b"CAGCATAC")])
def test_group_args_accepts_every_host_buffer(seqs):
    off, starts, lens, n_groups, n, h_ptr, d_ptr, buf = group_args(*GOOD, seqs, None, None)
    assert (off.dtype, starts.dtype, lens.dtype) == (np.int32, np.int64, np.int32)
    assert (off.tolist(), starts.tolist(), lens.tolist()) == tuple(list(a) for a in GOOD)
    assert n_groups == 2 and n == 8 and buf.dtype == np.uint8 and buf.tobytes() == b"CAGCATAC"
    assert h_ptr.value == buf.ctypes.data and d_ptr.value is None
    assert group_args(*GOOD, seqs, None, 5)[4] == 5                   # fewer bytes declared than the buffer has
    assert group_args(*GOOD, seqs, None, 8)[4] == 8


def test_group_args_device_buffer_and_no_groups():
    off, starts, lens, n_groups, n, h_ptr, d_ptr, buf = group_args(*GOOD, None, 0x7f0000001000, 8)
    assert n_groups == 2 and n == 8 and h_ptr.value is None and d_ptr.value == 0x7f0000001000 and buf is None
    off, starts, lens, n_groups, n, h_ptr, d_ptr, buf = group_args([0], [], [], b"", None, None)
    assert n_groups == 0 and n == 0 and off.tolist() == [0] and starts.shape == lens.shape == (0,) and h_ptr.value is None
    assert group_args([0, 0, 0], [], [], b"ACGT", None, None)[3:5] == (2, 4)      # empty groups span no sequence
