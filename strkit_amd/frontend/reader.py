"""Choosing and opening the reader of an alignment file given as a path: the decision as a pure function, and the opener
that inflates and scans the file on the device in the background while the caller's thread prepares the catalog."""
from __future__ import annotations

import os
import threading
import time

from .. import _lib
from .native import DeviceBam, IndexedBam, NativeBam, host_header

RESIDENT_FACTOR = 7.5           # device bytes per byte of a BGZF alignment file kept whole in HBM: the compressed bytes + ~6x
                                # decompressed (measured 5.8x on 30x HiFi data) + scan / extraction work buffers
STRK_E_NOMEM = -12
DEVICE_WHOLE, DEVICE_SPANS, HOST_INDEXED, HOST_STREAM = "device-whole", "device-spans", "host-indexed", "host-stream"


def _check_front_end(front_end: str) -> None:
    if front_end not in ("auto", "device", "host"):
        raise ValueError("front_end must be auto, device or host")


def choose_reader(front_end: str, file_bytes: int, free_mem: int, has_index: bool, distributed: bool) -> str:
    """Which reader a file gets.  Small = the compressed bytes plus their decompressed form (`RESIDENT_FACTOR` times the file)
    fit into 90 % of the device memory that is free right now.  On the GPU a small file is kept whole, a larger one goes through
    HBM span by span, which needs the index: without one the whole file is tried all the same (the opener falls back).  Under
    torch.distributed an indexed file is read in spans whatever its size: a rank's spans cover its own run of the catalog only."""
    _check_front_end(front_end)
    small = file_bytes * RESIDENT_FACTOR < 0.9 * free_mem
    if front_end == "device" or (front_end == "auto" and (small or has_index)):
        return DEVICE_WHOLE if (small and not (distributed and has_index)) or not has_index else DEVICE_SPANS
    return HOST_INDEXED if has_index else HOST_STREAM


def open_path(path: str, front_end: str, span_bytes: int, ctx, distributed: bool):
    """(reader, None) for a host reader, opened here, or (None, opener) for a device reader that opens in the background."""
    _check_front_end(front_end)                  # before the file is touched
    indexed = os.path.exists(path + ".bai") or os.path.exists(os.path.splitext(path)[0] + ".bai")
    # (the device of the rank, as _lib.default_context picks it — or the caller's context's: one process per GPU)
    dev = ctx.device if ctx is not None else int(os.environ.get("STRKIT_AMD_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    try:
        free_mem = _lib.device_mem(dev)[0]
    except Exception:  # noqa: BLE001  (no device: the reader reports it)
        free_mem = 0
    kind = choose_reader(front_end, os.path.getsize(path), free_mem, indexed, distributed)
    if kind in (DEVICE_WHOLE, DEVICE_SPANS):
        return None, BackgroundOpener(path, kind == DEVICE_WHOLE, dev, span_bytes, indexed).start()
    return (IndexedBam(path) if indexed else NativeBam(path)), None


class BackgroundOpener:
    # Opens a device reader in a thread of its own.  The file is opened (read, uploaded, inflated, scanned: reader threads and
    # the GPU, no Python) while the caller's thread loads the catalog and computes the reference side of every locus, which needs
    # neither.  What both need — the contig names — comes from the file's first blocks, inflated here (`references`).

    def __init__(self, path: str, whole: bool, device: int, span_bytes: int, indexed: bool):
        self.path, self.whole, self.device, self.span_bytes, self.indexed = path, whole, device, span_bytes, indexed
        self.references = [c for c, _ in host_header(path)[1]]
        self._reader = self._error = None
        self._seconds = 0.0
        self._thread = threading.Thread(target=self._open, name="strkit_amd-open")

    def _open(self):
        t0 = time.perf_counter()
        try:
            try:
                self._reader = DeviceBam(self.path, device=self.device, span_bytes=None if self.whole else self.span_bytes)
            except _lib.StrkError as e:
                if e.code != STRK_E_NOMEM:
                    raise
                # it did not fit after all (a file that inflates more than RESIDENT_FACTOR says): the whole file goes
                # through HBM in spans when it has an index; without one, or when even a span fails, the host reader
                if self.whole and self.indexed:
                    self._reader = DeviceBam(self.path, device=self.device, span_bytes=self.span_bytes)
                else:
                    self._reader = IndexedBam(self.path) if self.indexed else NativeBam(self.path)
        except BaseException as e:  # noqa: BLE001  (handed to the caller's thread by result())
            self._error = e
        self._seconds = time.perf_counter() - t0

    def start(self) -> "BackgroundOpener":
        self._thread.start()
        return self

    def result(self):
        """(reader, seconds the opening took, seconds this call still waited for it); raises what kept it from opening."""
        t0 = time.perf_counter()
        self._thread.join()
        if self._error is not None:
            raise self._error
        return self._reader, self._seconds, time.perf_counter() - t0

    def close_on_error(self) -> None:
        # the caller failed before it took the reader: do not leave one (gigabytes of device memory) behind
        self._thread.join()
        if isinstance(self._reader, DeviceBam):
            self._reader.close()
