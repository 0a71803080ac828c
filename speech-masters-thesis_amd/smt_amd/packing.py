"""Packed operand copies of the weights: who owns them, when they are refreshed and when they are thrown away.

Every conv needs its fp32 torch-layout weight in operand layout (twice: forward and data-gradient layouts).  Packing per use
costs ~390 tiny launches per train step.  Parameters keep their storage across optimiser steps, so each (weights, layout)
pair gets a persistent destination and a row in a device-side table, and ONE table-driven launch refreshes them all.  This
module knows nothing about convolutions: ``smt_amd.convops`` describes its layouts as lists of ``Part`` and calls ``pack``.

The rules, each stated once:

 1. Only ``nn.Parameter`` sources are cached, and they are held WEAKLY.  Any other source (weight-normed, padded or sliced
    weights: a new tensor every step) is packed on every use and never stored -- cached, it would pile up a dead entry
    per step (GlowTTS once reached 18 ms per repack that way).
 2. A single-part operand in the dense layout (``Part.dense``) goes through smt_pack_weight (by value: no table upload);
    anything else through a one-entry table.
 3. A key whose source has died is dropped; the new tensor that reuses the address gets a fresh entry.
 4. The first use of an entry packs only that entry.
 5. A later use while ``dirty``, or with a moved ``_version`` of a source, repacks ALL entries: one launch per device,
    inside the ``pack_weights_batched`` profiler region, reusing the device table unless the entry set has changed.
 6. Each repack-all clears ``dirty`` and adds one to ``repacks``.
 7. ``mark_dirty`` bumps ``generation``.  ``Tensor._version`` alone is NOT enough to notice an optimizer step: torch's
    fused AdamW updates the parameters without moving their version counters on this torch / ROCm build, and the convs
    would go on multiplying with the weights of step 0.  So every ``torch.optim.Optimizer.step`` of the process marks
    dirty (a global post-hook registered below, once), and so does ...
 8. ... the OUTERMOST training scope of a forward pass (``training_forward`` / ``forward_scope``): whatever wrote the
    parameters since -- an optimizer of the integrator's own making, ``p.data.copy_``, a kernel writing by pointer -- the
    first conv of the pass repacks from the fp32 masters.  Nested scopes do not mark again; an eval-mode scope is
    transparent (a training sub-module inside it still marks).
 9. At ``MAX_ENTRIES`` the cache prunes the entries of dead parameters; if it is still full it clears itself.
10. ``epoch`` moves exactly when an entry is dropped or the cache is cleared, never on invalidation.  A captured graph
    (``smt_amd.graph.GraphedStep``) holds a ``pin()`` and refuses to replay once the epoch has moved.

Why pruning an UNRELATED dead model invalidates a pinned graph: the repack launch the graph captured reads the device
table of that moment, and the table lists every entry of the cache -- the dead model's too, whose source storage has been
freed and may belong to anything by now.  The pin keeps the destinations and the table alive, not the sources.
"""
import contextlib
import ctypes
import functools
import weakref
from dataclasses import dataclass

import torch
from torch.optim.optimizer import register_optimizer_step_post_hook

from . import native as N
from . import profiler

DTYPE_CODE = {torch.float32: 0, torch.bfloat16: 1}      # SMT_F32, SMT_BF16 (include/smt_hip.h)


class PackEntry(ctypes.Structure):
    """Mirror of ``smt_pack_entry`` (include/smt_hip.h)."""
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("stride_out", ctypes.c_int64),
                ("stride_in", ctypes.c_int64), ("stride_tap", ctypes.c_int64), ("dst_offset", ctypes.c_int64),
                ("dst_tap_stride", ctypes.c_int64), ("dst_row_stride", ctypes.c_int64), ("dtype", ctypes.c_int),
                ("n_out", ctypes.c_int), ("n_in", ctypes.c_int), ("taps", ctypes.c_int), ("swizzle", ctypes.c_int),
                ("tap_map", ctypes.c_int * 16)]


@dataclass(slots=True)
class Part:
    """One source of an operand: dst[dst_offset + tap*dst_tap_stride + o*dst_row_stride + i'] =
    src[o*stride_out + i*stride_in + tap_map[tap]*stride_tap] for o < n_out, i < n_in (i' = i, or the LDS-DMA chunk
    position of i when ``swizzle``).  ``tap_map`` is a tuple: the part is hashed (``key``) on every use of the operand."""
    src: torch.Tensor
    n_out: int
    n_in: int
    stride_out: int
    stride_in: int
    stride_tap: int
    tap_map: tuple
    swizzle: bool
    dst_offset: int
    dst_tap_stride: int
    dst_row_stride: int

    @classmethod
    def dense(cls, src, n_out, n_in, stride_out, stride_in, stride_tap, tap_map, swizzle=False):
        """The common case, an operand of one part: the destination is [len(tap_map)][n_out][n_in], densely."""
        return cls(src, n_out, n_in, stride_out, stride_in, stride_tap, tuple(tap_map), bool(swizzle), 0, n_out * n_in, n_in)

    def is_dense(self):
        return (self.dst_offset, self.dst_tap_stride, self.dst_row_stride) == (0, self.n_out * self.n_in, self.n_in)

    def key(self):
        """What makes two parts the same cached copy: the source's address and shape, and the whole layout."""
        return (self.src.data_ptr(), self.src.shape, self.n_out, self.n_in, self.stride_out, self.stride_in,
                self.stride_tap, self.tap_map, self.swizzle, self.dst_offset, self.dst_tap_stride, self.dst_row_stride)

    def row(self, dst):
        assert self.src.dtype == torch.float32
        assert not self.swizzle or (dst.dtype == torch.bfloat16 and self.n_in % 128 == 0)
        return PackEntry(self.src.data_ptr(), dst.data_ptr(), self.stride_out, self.stride_in, self.stride_tap,
                         self.dst_offset, self.dst_tap_stride, self.dst_row_stride, DTYPE_CODE[dst.dtype], self.n_out,
                         self.n_in, len(self.tap_map), int(self.swizzle), (ctypes.c_int * 16)(*self.tap_map))


class _Entry:
    """One operand: its destination, and per part a weak reference to the source and the table row that packs it."""
    __slots__ = ("dst", "refs", "rows", "versions")

    def __init__(self, parts, dtype, dst_shape):
        self.dst = torch.empty(dst_shape, dtype=dtype, device=parts[0].src.device)
        self.refs = [weakref.ref(p.src) for p in parts]
        self.rows = [p.row(self.dst) for p in parts]
        self.versions = None     # the sources' version counters at the last pack

    def live_versions(self):
        """Version counters of the sources, or None if one of them has died."""
        out = []
        for ref in self.refs:
            src = ref()
            if src is None:
                return None
            out.append(src._version)
        return out


def _launch_one(e):
    """Pack a single-part operand in the dense layout by value (smt_pack_weight)."""
    pe, = e.rows
    assert e.dst.is_cuda
    taps = (ctypes.c_int * pe.taps)(*pe.tap_map[:pe.taps])
    N.check(N.lib().smt_pack_weight(ctypes.c_void_p(pe.src), ctypes.c_void_p(pe.dst), pe.dtype, pe.n_out, pe.n_in, pe.taps,
                                    pe.stride_out, pe.stride_in, pe.stride_tap, taps, pe.swizzle, N.stream_ptr()),
            "smt_pack_weight")


def _launch_table(entries, table=None):
    """Pack the operands of one device in one launch (smt_pack_weights_batched); returns the uploaded table, which the
    caller may pass back in for as long as ``entries`` stay the same."""
    if table is None:
        table = _upload(entries)
    rows_dev, blk_entry, blk_local, n_blocks = table
    assert rows_dev.is_cuda
    N.check(N.lib().smt_pack_weights_batched(ctypes.c_void_p(rows_dev.data_ptr()), ctypes.c_void_p(blk_entry.data_ptr()),
                                             ctypes.c_void_p(blk_local.data_ptr()), n_blocks, N.stream_ptr()),
            "smt_pack_weights_batched")
    return table


def _upload(entries):
    """(table rows, row of every block, index of every block within its row, number of blocks) on the entries' device:
    one block of the launch packs 1024 elements of one row."""
    rows, blk_entry, blk_local = [], [], []
    for e in entries:
        for pe in e.rows:
            nb = (pe.taps * pe.n_out * pe.n_in + 1023) // 1024
            blk_entry += [len(rows)] * nb
            blk_local += range(nb)
            rows.append(pe)
    dev = entries[0].dst.device
    table = torch.frombuffer(bytearray(bytes((PackEntry * len(rows))(*rows))), dtype=torch.uint8).to(dev)
    return (table, torch.tensor(blk_entry, dtype=torch.int32).to(dev), torch.tensor(blk_local, dtype=torch.int32).to(dev),
            len(blk_entry))


class PackCache:
    """The rules of the module docstring.  The process uses one instance (the module-level functions below)."""

    MAX_ENTRIES = 8192

    def __init__(self):
        self.entries = {}        # key -> _Entry, in table order
        self.tables = None       # {device: what _launch_table returned}; None = the entry set changed, upload again
        self.dirty = False       # repack at the next use whatever the versions say
        self.generation = 0      # number of mark_dirty() calls
        self.epoch = 0           # moves when copies are thrown away (rule 10)
        self.repacks = 0         # repack-all rounds so far

    def mark_dirty(self):
        self.dirty = True
        self.generation += 1

    def _drop(self, key):
        del self.entries[key]
        self.tables = None
        self.epoch += 1

    def prune(self):
        """Forget the copies of parameters that no longer exist."""
        for key in [k for k, e in self.entries.items() if e.live_versions() is None]:
            self._drop(key)

    def pack(self, parts, dtype, dst_shape):
        """``parts`` packed side by side into one operand of shape ``dst_shape`` (a tuple: it is part of the key)."""
        if not all(isinstance(p.src, torch.nn.Parameter) for p in parts):
            e = _Entry(parts, dtype, dst_shape)
            if len(parts) == 1 and parts[0].is_dense():
                _launch_one(e)
            else:
                _launch_table([e])
            return e.dst
        key = (dtype, dst_shape, *[p.key() for p in parts])
        e = self.entries.get(key)
        versions = None if e is None else e.live_versions()
        if e is not None and versions is None:               # the address was reused by a new tensor
            self._drop(key)
            e = None
        if e is None:
            if len(self.entries) >= self.MAX_ENTRIES:
                self.prune()
            if len(self.entries) >= self.MAX_ENTRIES:
                self.entries.clear()
                self.epoch += 1
            e = self.entries[key] = _Entry(parts, dtype, dst_shape)
            self.tables = None
            _launch_table([e])
            e.versions = e.live_versions()
        elif self.dirty or e.versions != versions:
            self.repack_all()
        return e.dst

    def repack_all(self):
        self.prune()
        by_dev = {}
        for e in self.entries.values():
            by_dev.setdefault(e.dst.device, []).append(e)
        if self.tables is None:
            self.tables = {}
        for dev, es in by_dev.items():
            with profiler.region("pack_weights_batched", bound="hbm"):
                self.tables[dev] = _launch_table(es, self.tables.get(dev))
            for e in es:
                e.versions = e.live_versions()
        self.dirty = False
        self.repacks += 1

    def pin(self):
        return Pin(self)


class Pin:
    """Keeps alive what a captured repack launch points at -- the packed copies of the moment and their device tables --
    and remembers the epoch they belong to."""

    def __init__(self, cache):
        self._cache, self._epoch = cache, cache.epoch
        self._refs = (list(cache.entries.values()), cache.tables)

    def valid(self):
        """False once a copy has been thrown away since (rule 10): the captured launch must not run any more."""
        return self._cache.epoch == self._epoch


_cache = PackCache()      # the process's cache; the rest of the build uses the names from here on and no attribute of it
pack, prune, pin = _cache.pack, _cache.prune, _cache.pin
repack_all = _cache.repack_all    # before a graph capture: also uploads the device tables (an upload cannot be captured)


def mark_dirty(*_args, **_kwargs):
    """The parameters have (or may have) changed: repack every operand copy at its next use (rules 5 and 7).  Nobody has
    to call this: training forwards and optimizer steps do."""
    _cache.mark_dirty()


def invalidate():
    """The parameters were written behind torch's back (``p.data.copy_`` as in ``EMA.swap``, ``load_checkpoint``): every
    packed copy is refreshed at its next use.  The copies themselves -- keyed by the parameters' storage, which such writes
    do not move -- stay where they are and the epoch does not move, so a captured graph that points at them stays valid."""
    _cache.mark_dirty()


def generation():
    """Moves whenever the parameters have or may have changed: other per-weight caches of this build key on it beside
    ``_version`` (smt_amd.vqtts.WeightSplit)."""
    return _cache.generation


def epoch():
    return _cache.epoch


def repacks():
    return _cache.repacks


def entry_count():
    return len(_cache.entries)


def _is_dirty(clear=False):
    """For tests: the dirty flag, optionally cleared ("nobody told the cache anything")."""
    dirty = _cache.dirty
    if clear:
        _cache.dirty = False
    return dirty


_forward_depth = 0


@contextlib.contextmanager
def training_forward(training=True):
    """Scope of one forward pass of a module of this build (rule 8): correct weights are a property of the model, not a
    contract with its caller."""
    global _forward_depth
    if not training:
        yield
        return
    if _forward_depth == 0:
        mark_dirty()
    _forward_depth += 1
    try:
        yield
    finally:
        _forward_depth -= 1


def forward_scope(forward):
    """Decorator form of ``training_forward`` for ``nn.Module.forward`` methods (reads ``self.training``)."""
    @functools.wraps(forward)
    def scoped(self, *args, **kwargs):
        with training_forward(self.training):
            return forward(self, *args, **kwargs)
    return scoped


register_optimizer_step_post_hook(mark_dirty)      # rule 7: every optimizer instance of the process, whoever builds it
