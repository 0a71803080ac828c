"""smt_pack_weights_batched and smt_pack_weight against the emulation of tests/pack_emulation.py -- the one
tests/test_packing_cpu.py runs the cache's rules on -- bit for bit (fp32 copies; fp32 -> bf16 rounds to nearest even on
both sides), for every operand layout of smt_amd.convops."""
import pytest
import torch

import pack_emulation as E

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16


def _cases():
    from smt_amd import convops as C
    w1 = [(128, 64, 1)] * 4
    return {
        "a_fwd_f32": ([(64, 32, 3)], lambda w: C._pack_fwd(w[0], F32)),
        "b_bwd_bf16_swizzled": ([(128, 128, 5)], lambda w: C._pack_bwd(w[0], BF16, swizzle=True)),
        "c_cat_fwd": (w1, lambda w: C._pack_cat_fwd(w, BF16)),
        "d_cat_fwd_swizzled": ([(128, 128, 1)] * 4, lambda w: C._pack_cat_fwd(w, BF16, swizzle=True)),
        "e_cat_bwd": (w1, lambda w: C._pack_cat_bwd(w, BF16)),
        "f_cat_bias": ([(128,)] * 4, lambda w: C._cat_bias(w)),
        "g_tap_subset": ([(64, 64, 4)], lambda w: C._pack(w[0], BF16, 64, 64, 4, 64 * 4, 1, [1, 3])),
    }


@pytest.mark.parametrize("source", ["parameter", "tensor"])
@pytest.mark.parametrize("case", ["a_fwd_f32", "b_bwd_bf16_swizzled", "c_cat_fwd", "d_cat_fwd_swizzled", "e_cat_bwd",
                                  "f_cat_bias", "g_tap_subset"])
def test_pack_kernels_equal_the_emulation_bit_for_bit(case, source, monkeypatch):
    """Parameters take the table launch (smt_pack_weights_batched); plain tensors the by-value launch (smt_pack_weight)
    where the operand is a single dense part, and a one-entry table otherwise."""
    shapes, build = _cases()[case]
    g = torch.Generator(device="cuda").manual_seed(len(case))
    ws = [torch.randn(*s, device="cuda", generator=g) for s in shapes]
    if source == "parameter":
        ws = [torch.nn.Parameter(w) for w in ws]
    launches = E.Launches(monkeypatch, emulate=False)
    out = build(ws)
    torch.cuda.synchronize()
    (kind, rows, _, _, (entry,)), = launches.log
    assert kind == ("one" if source == "tensor" and len(ws) == 1 else "table") and len(rows) == len(ws)
    assert entry.dst is out
    assert torch.equal(E.bits(out), E.bits(E.expected(entry)))
