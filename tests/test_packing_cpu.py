"""smt_amd.packing without a GPU: the cache's rules (the module docstring numbers them) are host policy, so they run on CPU
tensors with the two launch functions replaced by the emulation of tests/pack_emulation.py, which also records every
launch and the table rows it packed.  The layout helpers of smt_amd.convops are checked the same way against plain torch
expressions."""
import gc
import weakref

import pytest
import torch

import pack_emulation as E
from smt_amd import convops as C
from smt_amd import packing
from smt_amd.packing import Part

F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture
def launches(monkeypatch):
    return E.Launches(monkeypatch)


def param(*shape, seed=0):
    return torch.nn.Parameter(torch.randn(*shape, generator=torch.Generator().manual_seed(seed)))


def fwd_part(w):
    """The dense [k][c_out][c_in] operand of a [c_out, c_in, k] weight."""
    c_out, c_in, k = w.shape
    return Part.dense(w, c_out, c_in, c_in * k, k, 1, range(k))


def pack_fwd(cache, w, dtype=F32):
    return cache.pack([fwd_part(w)], dtype, (w.shape[2], w.shape[0], w.shape[1]))


def test_part_dense_is_the_dense_layout_and_parts_key_on_address_and_layout():
    w = param(6, 4, 3)
    p = fwd_part(w)
    assert (p.dst_offset, p.dst_tap_stride, p.dst_row_stride) == (0, 24, 4) and p.is_dense() and p.tap_map == (0, 1, 2)
    assert not Part(w, 6, 4, 12, 3, 1, (0,), False, 0, 48, 4).is_dense()
    assert p.key() == fwd_part(w).key() != Part.dense(w, 6, 4, 12, 3, 1, [2, 1, 0]).key()
    assert p.key() != fwd_part(param(6, 4, 3)).key()                       # another tensor, another address


def test_only_parameters_are_cached_and_they_are_held_weakly(launches):
    cache = packing.PackCache()
    plain = torch.randn(6, 4, 3)
    a, b = pack_fwd(cache, plain), pack_fwd(cache, plain)
    assert torch.equal(a, plain.permute(2, 0, 1)) and a.data_ptr() != b.data_ptr()
    assert len(cache.entries) == 0 and launches.kinds() == ["one", "one"]          # rule 1: packed on every use, never stored
    w = param(6, 4, 3)
    a, b = pack_fwd(cache, w), pack_fwd(cache, w)
    assert a.data_ptr() == b.data_ptr() and len(cache.entries) == 1 and len(launches.log) == 3
    alive = weakref.ref(w)
    del w
    gc.collect()
    assert alive() is None                                                         # the cache did not keep it alive


def test_by_value_launch_for_a_dense_single_part_and_a_one_entry_table_otherwise(launches):
    cache = packing.PackCache()
    w = torch.randn(6, 4, 1)
    pack_fwd(cache, w)
    cache.pack([Part(w, 6, 4, 4, 1, 1, (0,), False, 4, 40, 4)], F32, (1, 10, 4))                 # one part, not dense
    cache.pack([Part(w, 6, 4, 4, 1, 1, (0,), False, 0, 48, 4), Part(w, 6, 4, 4, 1, 1, (0,), False, 24, 48, 4)], F32, (1, 12, 4))
    assert launches.kinds() == ["one", "table", "table"]                                       # rule 2
    assert [len(rows) for _, rows, *_ in launches.log] == [1, 1, 2] and all(len(es) == 1 for *_, es in launches.log)


def test_a_dead_source_is_dropped_and_the_tensor_at_its_address_gets_a_fresh_entry(launches):
    cache = packing.PackCache()
    other = param(6, 4, 3, seed=1)
    pack_fwd(cache, other)
    storage = torch.randn(6, 4, 3)
    w = torch.nn.Parameter(storage)                     # shares the storage: a second Parameter of it has the same address
    first = pack_fwd(cache, w)
    (key, entry), = [(k, e) for k, e in cache.entries.items() if e.dst is first]
    epoch = cache.epoch
    del w
    gc.collect()
    with torch.no_grad():
        storage.mul_(2.0)
    w2 = torch.nn.Parameter(storage)
    n = len(launches.log)
    second = pack_fwd(cache, w2)
    assert cache.entries[key] is not entry and second is not first and len(cache.entries) == 2          # rule 3
    assert cache.epoch == epoch + 1                                                                     # rule 10: a drop
    assert torch.equal(second, w2.detach().permute(2, 0, 1))
    kind, rows, reused, _, entries = launches.log[-1]
    assert len(launches.log) == n + 1 and (kind, len(rows), reused) == ("table", 1, False)              # rule 4: only this one
    assert entries == [cache.entries[key]]


def test_dirty_or_a_moved_version_repacks_all_entries_in_one_launch(launches):
    cache = packing.PackCache()
    ws = [param(6, 4, 3, seed=s) for s in range(3)]
    outs = [pack_fwd(cache, w, BF16) for w in ws]
    assert [len(rows) for _, rows, *_ in launches.log] == [1, 1, 1] and cache.repacks == 0              # rule 4
    n = len(launches.log)
    assert pack_fwd(cache, ws[0], BF16) is outs[0] and len(launches.log) == n                            # clean: a cache hit
    epoch, generation = cache.epoch, cache.generation
    cache.mark_dirty()
    assert cache.dirty and cache.generation == generation + 1                                           # rule 7
    with torch.no_grad():
        for w in ws:
            w.data.mul_(-3.0)                           # behind torch's back: no version moves
    assert pack_fwd(cache, ws[1], BF16) is outs[1]
    kind, rows, reused, regions, _ = launches.log[-1]
    assert len(launches.log) == n + 1 and (kind, len(rows), reused) == ("table", 3, False)               # rule 5: one launch
    assert regions == ["pack_weights_batched"]
    assert not cache.dirty and cache.repacks == 1                                                        # rule 6
    assert all(torch.equal(o, w.detach().permute(2, 0, 1).to(BF16)) for o, w in zip(outs, ws))
    with torch.no_grad():
        ws[2].add_(1.0)                                 # a version moves; nobody marks anything
    assert pack_fwd(cache, ws[0], BF16) is outs[0] and len(launches.log) == n + 1                        # this entry's did not
    pack_fwd(cache, ws[2], BF16)
    kind, rows, reused, regions, _ = launches.log[-1]
    assert (kind, len(rows), reused, regions) == ("table", 3, True, ["pack_weights_batched"])            # the table is reused
    assert cache.repacks == 2 and torch.equal(outs[2], ws[2].detach().permute(2, 0, 1).to(BF16))
    extra = param(6, 4, 3, seed=9)
    pack_fwd(cache, extra, BF16)                        # the entry set changes: the next repack-all uploads a new table
    cache.mark_dirty()
    pack_fwd(cache, extra, BF16)
    kind, rows, reused, *_ = launches.log[-1]
    assert (kind, len(rows), reused) == ("table", 4, False) and cache.repacks == 3
    assert cache.epoch == epoch                                                                          # rule 10: never here


def test_overflow_prunes_first_and_clears_when_that_does_not_help(launches):
    cache = packing.PackCache()
    cache.MAX_ENTRIES = 3
    ws = [param(6, 4, 3, seed=s) for s in range(3)]
    for w in ws:
        pack_fwd(cache, w)
    epoch = cache.epoch
    del ws[0], w
    gc.collect()
    ws.append(param(6, 4, 3, seed=3))
    pack_fwd(cache, ws[-1])                             # full, but one entry is dead: pruning makes room
    assert len(cache.entries) == 3 and cache.epoch == epoch + 1                                          # rule 9, rule 10
    ws.append(param(6, 4, 3, seed=4))
    out = pack_fwd(cache, ws[-1])                       # full of live entries: everything goes
    assert len(cache.entries) == 1 and cache.epoch == epoch + 2
    assert torch.equal(out, ws[-1].detach().permute(2, 0, 1))


def test_only_the_outermost_training_scope_marks_dirty_and_the_optimizer_hook_is_registered_once():
    g0 = packing.generation()
    with packing.training_forward(True):
        with packing.training_forward(True):
            pass
    assert packing.generation() == g0 + 1 and packing._is_dirty()                                        # rule 8
    with packing.training_forward(False):
        pass
    assert packing.generation() == g0 + 1                                                                # eval: transparent
    with packing.training_forward(False):
        with packing.training_forward(True):
            pass
    assert packing.generation() == g0 + 2
    p = param(3)
    p.grad = torch.ones(3)
    torch.optim.SGD([p], lr=0.1).step()
    assert packing.generation() == g0 + 3                                                                # one hook, not two
    assert packing._is_dirty(clear=True) and not packing._is_dirty()


def test_a_pin_survives_invalidation_and_repacks_but_not_the_pruning_of_an_unrelated_parameter(launches):
    gc.collect()
    packing.prune()                                     # whatever earlier tests left behind goes now, not under the pin
    mine, unrelated = param(6, 4, 3, seed=1), param(5, 2, 1, seed=2)
    kept = C._pack_fwd(mine, BF16)
    C._pack_fwd(unrelated, F32)
    n = packing.entry_count()
    pin = packing.pin()
    epoch, repacks = packing.epoch(), packing.repacks()
    packing.invalidate()
    assert C._pack_fwd(mine, BF16) is kept and packing.repacks() == repacks + 1                          # a repack-all
    packing.repack_all()
    assert pin.valid() and packing.epoch() == epoch and packing.repacks() == repacks + 2
    del unrelated
    gc.collect()
    packing.prune()
    assert not pin.valid() and packing.epoch() == epoch + 1 and packing.entry_count() == n - 1
    assert C._pack_fwd(mine, BF16) is kept                                   # the live copy itself stays where it was


def test_layout_helpers_build_the_operands_the_kernels_expect(launches):
    """Parameters (table launches) and plain tensors (by-value launch where the operand is one dense part) alike."""
    for wrap in (torch.nn.Parameter, lambda t: t):
        w = wrap(torch.randn(10, 6, 5))
        assert torch.equal(C._pack_fwd(w, F32), w.detach().permute(2, 0, 1))
        assert torch.equal(C._pack_bwd(w, BF16), w.detach().flip(2).permute(2, 1, 0).to(BF16))        # [tap][ci][co], taps flipped
        ws = [wrap(torch.randn(o, 6, 1)) for o in (4, 2, 7)]
        assert torch.equal(C._pack_cat_fwd(ws, F32), torch.cat([x.detach()[:, :, 0] for x in ws], 0)[None])
        assert torch.equal(C._pack_cat_bwd(ws, BF16), torch.cat([x.detach()[:, :, 0].t() for x in ws], 1)[None].to(BF16))
        bs = [wrap(torch.randn(o)) for o in (4, 2, 7)]
        assert torch.equal(C._cat_bias(bs), torch.cat([x.detach() for x in bs]).view(1, 13, 1))
        wt = wrap(torch.randn(6, 10, 4))                # ConvTranspose1d layout [c_in, c_out, k]; one operand per output phase
        for taps, _ in C._phases(4, 2, 1):
            assert sorted(taps) in ([1, 3], [0, 2])
            assert torch.equal(C._pack(wt, F32, 10, 6, 4, 40, 1, taps), wt.detach()[:, :, taps].permute(2, 1, 0))
    kinds = launches.kinds()
    half = len(kinds) // 2
    assert set(kinds[:half]) == {"table"} and kinds[half:] == ["one", "one", "table", "table", "table", "one", "one"]


def test_swizzled_operands_swap_chunks_within_groups_of_128_input_channels(launches):
    """Chunk c (8 channels) of row o sits at chunk c ^ (o & 15) of its group of 128: an involution, so the same gather undoes it."""
    ws = [torch.nn.Parameter(torch.randn(32, 256, 1)) for _ in range(2)]
    plain, swz = C._pack_cat_fwd(ws, BF16), C._pack_cat_fwd(ws, BF16, swizzle=True)
    o = torch.arange(32)
    chunk = torch.arange(16)[None, :] ^ (o & 15)[:, None]                                     # [o][c] -> source chunk
    for d in range(2):
        part = plain[0, 32 * d:32 * d + 32].view(32, 2, 16, 8)
        moved = torch.gather(part, 2, chunk[:, None, :, None].expand(32, 2, 16, 8))
        assert torch.equal(swz[0, 32 * d:32 * d + 32], moved.reshape(32, 256))
    assert torch.equal(C._pack_fwd(ws[0], BF16, swizzle=True), swz[:, :32])
