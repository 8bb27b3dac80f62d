"""Device -> Arrow result bridge (the blocking-node
result path core.py:455-482 / quokka_dataset.py).

Round 1 returned results through the generic pageable bounce
(DevColumn.to_numpy: DMA into a pinned staging chunk, then a host memmove
into the pageable numpy array Arrow wraps — measured ~17 GB/s d2h). This
module removes the second copy: the DESTINATION buffer itself is pinned
host memory (hipHostMalloc), the DMA engine writes straight into it, and
pyarrow wraps it zero-copy (the numpy array IS the Arrow buffer; a
finalizer frees the pinned allocation when the last reference drops).
One DMA, no memmove — d2h at full PCIe rate.
"""
import ctypes
import weakref

import numpy as np

from . import shim
from .shim import c_u64, c_vp


class _PinnedPool:
    """Size-class free list for pinned host blocks. hipHostMalloc PINS
    pages — measured ~6.7 GB/s *effective* d2h when every result buffer
    is pinned fresh (the pinning dominates), vs the pure-DMA rate once
    blocks are recycled. Sizes round up to powers of two so repeated
    result shapes reuse blocks; capped, FIFO-evicting."""

    def __init__(self, cap_bytes=8 << 30):
        self.cap = cap_bytes
        self.cached = 0
        self.buckets = {}

    @staticmethod
    def size_class(nbytes):
        c = 4096
        while c < nbytes:
            c <<= 1
        return c

    def get(self, nbytes):
        lst = self.buckets.get(nbytes)
        if lst:
            self.cached -= nbytes
            return lst.pop()
        return None

    def put(self, nbytes, addr):
        if self.cached + nbytes > self.cap:
            shim._lib.qk_hfree(c_vp(addr))
            return
        self.buckets.setdefault(nbytes, []).append(addr)
        self.cached += nbytes


_pinned_pool = _PinnedPool()


class PinnedArray:
    """numpy array over pinned (hipHostMalloc) memory, recycled through
    _pinned_pool; a weakref finalizer returns the block when the array
    (and anything wrapping it, e.g. an Arrow buffer) is collected."""

    def __init__(self, dtype, n):
        dtype = np.dtype(dtype)
        nbytes = max(1, int(n) * dtype.itemsize)
        cls = _PinnedPool.size_class(nbytes)
        addr = _pinned_pool.get(cls)
        if addr is None:
            p = c_vp(0)
            shim.call("qk_hmalloc_impl", c_u64(cls), ctypes.byref(p))
            addr = p.value
        self.ptr = c_vp(addr)
        buf = (ctypes.c_byte * nbytes).from_address(addr)
        self.arr = np.frombuffer(buf, dtype=dtype, count=int(n))
        # the view chain (arrow Buffer -> numpy -> ctypes buf) keeps `buf`
        # alive; recycle the block only when that chain is gone
        weakref.finalize(buf, _pinned_pool.put, cls, addr)


def to_pinned_numpy(col, n=None, stream=None):
    """DevColumn -> numpy over a pinned buffer (one DMA, no memmove).
    Drop-in for DevColumn.to_numpy on result paths: pyarrow wraps the
    returned array zero-copy, so a pa.table() built from it references
    the DMA-written pinned memory directly."""
    n = col.n if n is None else int(n)
    pin = PinnedArray(col.dtype, n)
    if n:
        sh = stream.handle if stream else None
        shim.call("qk_d2h_async", sh, pin.ptr, col.ptr,
                  c_u64(n * col.dtype.itemsize))
        shim.call("qk_stream_sync", sh)
    return pin.arr


def column_to_arrow(col, n=None, stream=None):
    """One DevColumn -> pyarrow.Array over a pinned buffer (single DMA,
    zero host copies). An ops.NullableColumn keeps its nulls: the device
    bitmap is already in Arrow's validity layout, so it is copied to a
    pinned buffer like the values and wrapped as the validity buffer."""
    import pyarrow as pa
    from .ops import NullableColumn
    n = col.n if n is None else int(n)
    pin = PinnedArray(col.dtype, n)
    sh = stream.handle if stream else None
    vbuf, null_count = None, -1       # -1: pyarrow's own default
    if isinstance(col, NullableColumn):
        if n != col.n:
            raise ValueError("a NullableColumn converts whole (n=%d, "
                             "asked %d)" % (col.n, n))
        null_count = col.null_count
        vpin = PinnedArray(np.uint8, (n + 7) // 8)
        if n:
            shim.call("qk_d2h_async", sh, vpin.ptr, col.valid.ptr,
                      c_u64((n + 7) // 8))
        vbuf = pa.py_buffer(vpin.arr)
    if n:
        shim.call("qk_d2h_async", sh, pin.ptr, col.ptr,
                  c_u64(n * col.dtype.itemsize))
        shim.call("qk_stream_sync", sh)
    return pa.Array.from_buffers(
        pa.from_numpy_dtype(col.dtype), n,
        [vbuf, pa.py_buffer(pin.arr)], null_count=null_count)


def table_to_arrow(cols, stream=None):
    """dict name -> DevColumn  =>  pyarrow.Table (each column one direct
    DMA into its own pinned Arrow buffer). The reference's executors hand
    host Arrow back to the runtime (core.py:455-482); this is that
    boundary at PCIe rate."""
    import pyarrow as pa
    arrays = {name: column_to_arrow(c, stream=stream)
              for name, c in cols.items()}
    return pa.table(arrays)
