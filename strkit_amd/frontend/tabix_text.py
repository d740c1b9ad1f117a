"""A BGZF-compressed text file with a tabix index, read range by range: what IndexedSnvVcf (frontend/snv_vcf.py) and
IndexedAnnotations (frontend/annotations.py) share.  TabixText holds the index, the compressed bytes, the optional strk_dbam
object and the counters, and walks a byte range of the file in pieces of about `piece_bytes` decompressed bytes (`walk`): each
piece is inflated on the device or on the host cores and handed to the reader's `consume`, which parses it through the library and
says where its last complete line ended."""
from __future__ import annotations

import ctypes as C
import struct

import numpy as np

__all__ = ["TabixText"]


def _bgzf_block_bytes(comp: np.ndarray, off: int) -> tuple[int, int]:
    """(compressed size, decompressed size) of the BGZF block at compressed offset `off`."""
    if off + 18 > comp.size or comp[off] != 0x1F or comp[off + 1] != 0x8B or not comp[off + 3] & 4:
        raise ValueError(f"not a BGZF block at byte {off}")
    xlen = int(comp[off + 10]) | int(comp[off + 11]) << 8
    x, bsize = off + 12, -1
    while x + 4 <= off + 12 + xlen <= comp.size:
        slen = int(comp[x + 2]) | int(comp[x + 3]) << 8
        if comp[x] == 66 and comp[x + 1] == 67 and slen == 2:
            bsize = int(comp[x + 4]) | int(comp[x + 5]) << 8
        x += 4 + slen
    if bsize < 0 or off + bsize + 1 > comp.size:
        raise ValueError(f"truncated BGZF block at byte {off}")
    isize, = struct.unpack("<I", comp[off + bsize - 3:off + bsize + 1].tobytes())
    return bsize + 1, isize


class TabixText:
    """front_end="device": a strk_dbam object of its own holds the inflated piece in HBM; "host": strk_bgzf_inflate_range into a
    host buffer.  `preset`: the TabixIndex preset ("vcf" or "gff")."""

    def __init__(self, path: str, index: str, front_end: str, device: int, piece_bytes: int, tile_bytes: int, preset: str):
        from .tabix import TabixIndex
        if front_end not in ("host", "device"):
            raise ValueError(f"front_end must be 'host' or 'device', not {front_end!r}")
        self._precondition(path, index)
        self.path, self.front_end, self.piece_bytes, self.tile_bytes = path, front_end, int(piece_bytes), int(tile_bytes)
        self.index = TabixIndex(index, path, preset=preset)
        self.comp = np.memmap(path, np.uint8, "r")
        self.compressed_bytes = 0        # compressed bytes inflated so far (a block inflated twice counts twice)
        self.n_queries = 0
        self.seconds = 0.0
        self.text_bytes = 0              # decompressed bytes handed to the parser
        self.kernel_ms = [0.0, 0.0]      # device: HIP-event time of the inflation kernel, of the reader's kernels
        self._h = None
        if front_end == "device":
            from .. import _lib
            h = C.c_void_p()
            _lib.check(_lib.load().strk_dbam_open(int(device), C.byref(h)))
            self._h = h

    def _precondition(self, path: str, index: str) -> None:
        """What a reader wants of the two files before they are opened (raises ValueError); nothing here."""

    @property
    def references(self) -> list[str]:
        return list(self.index.names)

    def kernel_s(self) -> float:
        from .. import _lib
        return float(_lib.load().strk_dbam_kernel_ms(self._h)) / 1e3 if self._h is not None else 0.0

    def close(self) -> None:
        if self._h is not None:
            from .. import _lib
            _lib.load().strk_dbam_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _piece(self, coff: int, limit: int, want: int) -> tuple[list[int], list[int], int]:
        """The blocks from `coff` on that a piece takes: at least one, then as long as the piece stays within `want` decompressed
        bytes and below `limit` -> (their compressed offsets, where each starts in the piece, the offset of the next block)."""
        coffs, outs, total, nxt = [], [], 0, coff
        while nxt < limit:
            csize, isize = _bgzf_block_bytes(self.comp, nxt)
            if coffs and total + isize > want:
                break
            coffs.append(nxt)
            outs.append(total)
            total += isize
            nxt += csize
        outs.append(total)
        return coffs, outs, nxt

    def _only_empty(self, coff: int) -> bool:
        while coff < self.comp.size:
            csize, isize = _bgzf_block_bytes(self.comp, coff)
            if isize:
                return False
            coff += csize
        return True

    def walk(self, rng, consume) -> None:
        """The byte range `rng` of the file (virtual offset of its first line, compressed offset of its last block: what the index
        names), piece by piece.  consume(buf, n, start, final) reads the text [start, n) of a piece (`buf`: the host buffer, None
        on the device, where the strk_dbam object holds it; `final`: the text ends its file) and returns (end_off, past): the
        offset just past the last complete line, and whether nothing wanted can follow.  A piece resumes at the block that holds
        the first line the piece before left incomplete."""
        from .. import _lib
        L = _lib.load()
        voff, last = rng
        coff, start = voff >> 16, voff & 0xFFFF
        limit = min(self.comp.size, last + _bgzf_block_bytes(self.comp, last)[0]) if last < self.comp.size else self.comp.size
        want = self.piece_bytes
        buf = None
        while coff < limit:
            coffs, outs, nxt = self._piece(coff, limit, want)
            n = outs[-1]
            self.compressed_bytes += nxt - coff
            got = C.c_int64(0)
            if self._h is not None:
                ms0 = L.strk_dbam_kernel_ms(self._h)
                r = L.strk_dbam_inflate(self._h, self.comp.ctypes.data, nxt, coff, max(n, 1), C.byref(got))
                ms1 = L.strk_dbam_kernel_ms(self._h)
                self.kernel_ms[0] += ms1 - ms0
            else:
                if buf is None or buf.size < n + 16:
                    buf = np.empty(n + 16, np.uint8)
                r = L.strk_bgzf_inflate_range(self.comp.ctypes.data, nxt, coff, buf.ctypes.data, buf.size, C.byref(got), 0)
            if r < 0:
                _lib.check(int(r))
            if int(r) != n or got.value != nxt:
                raise ValueError(f"{self.path}: the blocks at byte {coff} inflate to {int(r)} bytes, their headers say {n}")
            # the text ends its file when nothing but empty blocks (the EOF marker) follows
            final = int(self._only_empty(nxt))
            self.text_bytes += n - start
            try:
                end_off, past = consume(buf, n, start, final)
            except _lib.StrkError as e:
                raise _lib.StrkError(e.code, f"{self.path} (text inflated from compressed byte {coff}): {e}") from None
            if self._h is not None:
                self.kernel_ms[1] += L.strk_dbam_kernel_ms(self._h) - ms1
            if past or nxt >= limit:        # (a line cut off by the range's last block begins past every wanted record)
                break
            if end_off >= n:                # the piece ended on a line end
                coff, start, want = nxt, 0, self.piece_bytes
                continue
            b = int(np.searchsorted(outs[:-1], end_off, side="right")) - 1
            if coffs[b] == coff and end_off - outs[b] == start:
                want = max(2 * want, 2 * n)     # not one complete line in the piece: a longer one
            else:
                coff, start, want = coffs[b], end_off - outs[b], self.piece_bytes
