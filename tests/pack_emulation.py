"""The weight-pack kernels restated from their definition (include/smt_hip.h, "Repack an fp32 torch-layout weight"):

    dst[dst_offset + tap*dst_tap_stride + o*dst_row_stride + ipos] = src[o*stride_out + i*stride_in + tap_map[tap]*stride_tap]
    ipos = i, or with swizzle (i & ~127) | ((((i >> 3) & 15) ^ (o & 15)) << 3) | (i & 7)

in torch indexing, on whatever device the tensors live (fp32 -> bf16 is round-to-nearest-even on both sides, so a kernel
must agree bit for bit), and stand-ins for the two launch functions of smt_amd.packing that run it and record every launch.
"""
import contextlib
import ctypes

import torch

from smt_amd import packing


def emulate_row(src, row, dst):
    """Pack one table row (a ``packing.PackEntry``; its two pointers are ``src`` and ``dst``) into ``dst``."""
    assert (row.src, row.dst, row.dtype) == (src.data_ptr(), dst.data_ptr(), packing.DTYPE_CODE[dst.dtype])
    taps = list(row.tap_map[:row.taps])
    # as_strided refuses a view that reaches outside the source's storage: the bounds check of the row
    view = src.detach().as_strided((row.n_out, row.n_in, max(taps) + 1), (row.stride_out, row.stride_in, row.stride_tap))
    tap, o, i = torch.meshgrid(torch.arange(row.taps), torch.arange(row.n_out), torch.arange(row.n_in), indexing="ij")
    ipos = (i & ~127) | ((((i >> 3) & 15) ^ (o & 15)) << 3) | (i & 7) if row.swizzle else i
    index = row.dst_offset + tap * row.dst_tap_stride + o * row.dst_row_stride + ipos
    assert 0 <= int(index.min()) and int(index.max()) < dst.numel() and index.unique().numel() == index.numel()
    dst.view(-1)[index.to(dst.device)] = view[:, :, taps].permute(2, 0, 1).to(dst.dtype)


def expected(entry):
    """What the launch that packed ``entry`` must have left in ``entry.dst``, in a tensor of its own."""
    out = torch.zeros_like(entry.dst)
    for ref, row in zip(entry.refs, entry.rows):
        fake = packing.PackEntry.from_buffer_copy(row)
        fake.dst = out.data_ptr()
        emulate_row(ref(), fake, out)
    return out


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


class Launches:
    """Stand-ins for ``packing._launch_one`` / ``packing._launch_table``, put in place through ``monkeypatch``.

    ``emulate=True``: nothing native runs; the table launch packs the rows of the TABLE it was given -- decoded from the
    uploaded bytes, so a stale cached table shows -- and every address in it must belong to a live tensor of ``entries``.
    ``emulate=False``: the real launch runs and is only recorded.
    ``log`` holds one (kind, rows, table_reused, open profiler regions, entries) per launch."""

    def __init__(self, monkeypatch, emulate=True):
        self.log, self.regions, self.emulate = [], [], emulate
        self.real = (packing._launch_one, packing._launch_table)
        monkeypatch.setattr(packing, "_launch_one", self.one)
        monkeypatch.setattr(packing, "_launch_table", self.table)
        monkeypatch.setattr(packing.profiler, "region", self.region)

    @contextlib.contextmanager
    def region(self, name, **_):
        self.regions.append(name)
        try:
            yield
        finally:
            self.regions.pop()

    def one(self, e):
        row, = e.rows
        if self.emulate:
            emulate_row(e.refs[0](), row, e.dst)
        else:
            self.real[0](e)
        self.log.append(("one", [row], False, list(self.regions), [e]))

    def table(self, entries, table=None):
        reused = table is not None
        if not self.emulate:
            table = self.real[1](entries, table)
            rows = [r for e in entries for r in e.rows]
        else:
            if table is None:
                table = packing._upload(entries)
            raw, blk_entry, blk_local, n_blocks = table
            rows = list((packing.PackEntry * (raw.numel() // ctypes.sizeof(packing.PackEntry)))
                        .from_buffer_copy(raw.numpy().tobytes()))
            blocks = [(r.taps * r.n_out * r.n_in + 1023) // 1024 for r in rows]      # 1024 elements per block
            assert blk_entry.tolist() == [j for j, nb in enumerate(blocks) for _ in range(nb)]
            assert blk_local.tolist() == [b for nb in blocks for b in range(nb)] and n_blocks == sum(blocks)
            tensors = {}
            for e in entries:
                tensors[e.dst.data_ptr()] = e.dst
                tensors.update((ref().data_ptr(), ref()) for ref in e.refs)
            for r in rows:
                emulate_row(tensors[r.src], r, tensors[r.dst])
        self.log.append(("table", rows, reused, list(self.regions), list(entries)))
        return table

    def kinds(self):
        return [kind for kind, *_ in self.log]
