"""GlowTTS kernels (csrc/glow.hip, smt_amd/glow.py) one by one against float64 restatements of the reference's formulas, at
tiny shapes, at shapes that cross each tiling / grid-stride boundary of the kernels, and at BASELINE.json configs[4] sizes
(hidden 192, 160 flow channels, T_x ~ 200, T_y ~ 870).  Every check is a max-abs error scaled by the tensor's max magnitude,
so an error confined to a few rows (the lens[b] boundary, the edge of the relative-attention window, the last partial chunk
of a reduction) fails.  The padding contract ("rows >= len read as zero") is pinned for every op that takes
lens: padded rows holding finite garbage or NaN must not reach any valid row, reduction or parameter gradient."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import glow_oracle as go
from oracle import vqvae_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32_TOL = 1e-5      # fp32 FMA chains of a few terms, relative to the tensor's max magnitude
SUM_TOL = 1e-4      # long fp32 sums (hundreds of thousands of rows, T keys) and softmax-backward cancellation (dP - sum P dP)


def close(got, ref, tol, what=""):
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    err, scale = float((got - ref).abs().max()) if got.numel() else 0.0, float(ref.abs().max()) if ref.numel() else 0.0
    assert err <= tol * scale + 1e-12, f"{what}: max-abs error {err:.3e} > {tol:.0e} x max {scale:.3e}"


def gen(seed):
    return torch.Generator().manual_seed(seed)


def valid(lens, t):
    """[B, T, 1] bool: row t of item b is valid."""
    return (torch.arange(t)[None, :] < lens.cpu()[:, None]).unsqueeze(-1)


def pad_as(x, lens, fill):
    """x with the rows t >= lens[b] replaced by `fill` (a float, or 'garbage' = +-1e3)."""
    keep = valid(lens, x.shape[1]).to(x.device)
    if fill == "garbage":
        g = (torch.rand(x.shape, generator=gen(99)) * 2e3 - 1e3).to(x.device, x.dtype)
        return torch.where(keep, x, g)
    return torch.where(keep, x, torch.full_like(x, fill))


def cuda(*ts):
    return [t.float().to(DEV).contiguous() for t in ts]


def i32(lens):
    return lens.to(torch.int32).to(DEV)


def bits_equal(a, b, what):
    assert torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32)), f"{what}: not bit-identical to the zero-padded run"


def drop_keep(seed, site, n, p):
    """float64 factors keep(i) / (1 - p) of the counter-based generator (include/smt_hip.h "dropout") for linear index i < n."""
    keep = orc.dropout_keep_ntc(seed, site, 1, n, 1, p).reshape(-1)
    return torch.from_numpy(keep.astype(np.float64)) / (1.0 - p)


def make_drop(p, seed=11, site=3):
    from smt_amd.lm import Drop
    return Drop(p, True, seed, site)


# ------------------------------------------------------------------------------------------------ ActNorm
ACTNORM_SHAPES = [  # B, T, C, lens
    (1, 1, 8, [1]),
    (4, 37, 8, [37, 1, 0, 20]),
    (3, 90001, 8, [90001, 1, 88888]),     # 270,003 rows > GL_ROWS * 4096 (4,219 chunks, last one partial); 2.16 M elements > one grid
    (3, 435, 160, [435, 1, 300]),         # configs[4]: 160 flow channels, T_y 870 squeezed by 2
]


def _actnorm_ref(x, logs, bias, lens, reverse):
    m = valid(lens, x.shape[1]).double().transpose(1, 2)
    p = {"a.logs": logs.view(1, -1, 1), "a.bias": bias.view(1, -1, 1)}
    z, _ = go.actnorm(x.transpose(1, 2), m, p, "a", reverse)
    return z.transpose(1, 2)


@pytest.mark.parametrize("b,t,c,lens", ACTNORM_SHAPES)
def test_actnorm_forward_reverse_backward(b, t, c, lens):
    from smt_amd import glow
    g = gen(1)
    x, dz = torch.randn(b, t, c, generator=g), torch.randn(b, t, c, generator=g) + 0.5     # mean 0.5: column sums ~ rows, not ~ sqrt(rows)
    logs, bias = 0.3 * torch.randn(c, generator=g), torch.randn(c, generator=g)
    lens = torch.tensor(lens)
    dz = dz * valid(lens, t)
    x64, logs64, bias64 = (a.double().requires_grad_(True) for a in (x * valid(lens, t), logs, bias))
    z_ref = _actnorm_ref(x64, logs64, bias64, lens, False)
    z_ref.backward(dz.double())
    xd, ld, bd, dzd = cuda(x, logs, bias, dz)
    xd.requires_grad_(True); ld.requires_grad_(True); bd.requires_grad_(True)
    z = glow.actnorm(xd, ld, bd, i32(lens))
    z.backward(dzd)
    close(z, z_ref.detach(), F32_TOL, "z")
    close(xd.grad, x64.grad, F32_TOL, "dx")
    close(ld.grad, logs64.grad, SUM_TOL if b * t > 1000 else F32_TOL, "dlogs")
    close(bd.grad, bias64.grad, SUM_TOL if b * t > 1000 else F32_TOL, "dbias")
    zr = glow.actnorm_reverse(xd.detach(), ld.detach(), bd.detach(), i32(lens))
    close(zr, _actnorm_ref(x.double(), logs.double(), bias.double(), lens, True), F32_TOL, "reverse")
    back = glow.actnorm_reverse(z.detach(), ld.detach(), bd.detach(), i32(lens))
    close(back, x.double() * valid(lens, t), F32_TOL, "reverse(forward(x))")


@pytest.mark.parametrize("b,t,c,lens", ACTNORM_SHAPES)
def test_masked_channel_moments(b, t, c, lens):
    """(count, sum x, sum x^2) over the valid rows: dz = 1 reaches the padded rows here, so the lens boundary shows directly."""
    from smt_amd import glow
    x = torch.randn(b, t, c, generator=gen(2)) + 1.0
    lens = torch.tensor(lens)
    cnt, s1, s2 = glow.masked_channel_moments(pad_as(x, lens, "garbage").to(DEV), i32(lens))
    m = valid(lens, t).double()
    x64 = x.double() * m
    close(cnt, m.sum((0, 1)).expand(c), 0.0, "count")
    close(s1, x64.sum((0, 1)), SUM_TOL if b * t > 1000 else F32_TOL, "sum x")
    close(s2, (x64 ** 2).sum((0, 1)), SUM_TOL if b * t > 1000 else F32_TOL, "sum x^2")


# ------------------------------------------------------------------------------------------------ InvConvNear
INVCONV_SHAPES = [(2, 5, 4, [5, 1]), (3, 29, 8, [29, 0, 1]), (3, 90001, 8, [90001, 1, 77777]), (3, 435, 160, [435, 1, 300])]


def _invconv_ref(x, w, lens, reverse=False):
    m = valid(lens, x.shape[1]).double().transpose(1, 2)
    z, _ = go.invconv(x.transpose(1, 2), m, {"w.weight": w}, "w", 4, reverse)
    return z.transpose(1, 2)


@pytest.mark.parametrize("b,t,c,lens", INVCONV_SHAPES)
def test_invconv_forward_reverse_weight_gradient(b, t, c, lens):
    from smt_amd import glow
    g = gen(3)
    x, dz = torch.randn(b, t, c, generator=g), torch.randn(b, t, c, generator=g) + 0.5
    w, _ = torch.linalg.qr(torch.randn(4, 4, generator=g))
    w = w + 0.1 * torch.randn(4, 4, generator=g)                # not orthogonal: the transpose in the backward matters
    lens = torch.tensor(lens)
    dz = dz * valid(lens, t)
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    z_ref = _invconv_ref(x64, w64, lens)
    z_ref.backward(dz.double())
    xd, wd, dzd = cuda(x, w, dz)
    xd.requires_grad_(True); wd.requires_grad_(True)
    z = glow.invconv(xd, wd, i32(lens))
    z.backward(dzd)
    close(z, z_ref.detach(), F32_TOL, "z")
    close(xd.grad, x64.grad, F32_TOL, "dx")
    close(wd.grad, w64.grad, SUM_TOL if b * t > 1000 else F32_TOL, "dW")
    w_inv = torch.inverse(w.double())
    back = glow.invconv_reverse(z.detach(), w_inv.float().to(DEV), i32(lens))
    close(back, x.double() * valid(lens, t), 1e-4, "reverse(forward(x))")   # through an fp32 inverse of a 4 x 4 matrix


# ------------------------------------------------------------------------------------------------ WN gate and dropout
@pytest.mark.parametrize("rows,h", [(1, 1), (7, 3), (2 * 435, 192), (4 * 1500, 192)])   # 4 * 1500 * 192 = 1.15 M > one grid
@pytest.mark.parametrize("p", [0.0, 0.05])
def test_wn_gate_forward_backward(rows, h, p):
    from smt_amd import glow
    g = gen(4)
    a, dacts = 2 * torch.randn(rows, 2 * h, generator=g), torch.randn(rows, h, generator=g)
    drop = make_drop(p) if p > 0 else make_drop(0.0)
    keep = drop_keep(11, 3, rows * 2 * h, p).view(rows, 2 * h) if p > 0 else torch.ones(rows, 2 * h, dtype=torch.float64)
    a64 = a.double().requires_grad_(True)
    ad = a64 * keep
    ref = torch.tanh(ad[:, :h]) * torch.sigmoid(ad[:, h:])
    ref.backward(dacts.double())
    ag = a.to(DEV).requires_grad_(True)
    acts = glow.wn_gate(ag, drop)
    acts.backward(dacts.to(DEV))
    close(acts, ref.detach(), F32_TOL, "acts")
    close(ag.grad, a64.grad, F32_TOL, "da")


@pytest.mark.parametrize("n", [1, 1000, 4096 * 256 + 77])
def test_dropout_mask_and_backward(n):
    from smt_amd import glow
    p = 0.1
    x = torch.randn(n, generator=gen(5)) + 3.0                  # nonzero everywhere: a zero output is a dropped element
    drop = make_drop(p, seed=5, site=7)
    keep = drop_keep(5, 7, n, p)
    xd = x.to(DEV).requires_grad_(True)
    y = glow.dropout(xd, drop)
    assert torch.equal(y.detach().cpu() == 0, keep == 0), "dropout mask differs from the counter spec"
    close(y, x.double() * keep, F32_TOL, "y")
    dy = torch.randn(n, generator=gen(6))
    y.backward(dy.to(DEV))
    close(xd.grad, dy.double() * keep, F32_TOL, "dx")


# ------------------------------------------------------------------------------------------------ affine coupling
COUPLING_SHAPES = [(1, 1, 4, [1]), (3, 130, 8, [130, 1, 0]), (3, 435, 160, [435, 1, 300]), (2, 140001, 8, [140001, 64])]   # 1.12 M half-rows: the backward's grid-stride loop


def _coupling_ref(out, x, lens, sig, reverse=False):
    m = valid(lens, x.shape[1]).double()
    h = x.shape[-1] // 2
    mm, logs = out[..., :h], out[..., h:]
    if sig:
        logs = torch.log(1e-6 + torch.sigmoid(logs + 2))
    if reverse:
        return torch.cat([x[..., :h], (x[..., h:] - mm) * torch.exp(-logs) * m], -1), None
    return torch.cat([x[..., :h], (mm + torch.exp(logs) * x[..., h:]) * m], -1), (logs * m).sum((1, 2))


@pytest.mark.parametrize("b,t,c,lens", COUPLING_SHAPES)
@pytest.mark.parametrize("sig", [False, True])
def test_coupling_forward_backward_reverse(b, t, c, lens, sig):
    from smt_amd import glow
    g = gen(7)
    out, x = 0.5 * torch.randn(b, t, c, generator=g), torch.randn(b, t, c, generator=g)
    dz, dld = torch.randn(b, t, c, generator=g), torch.randn(b, generator=g)
    lens = torch.tensor(lens)
    dz = dz * valid(lens, t)
    o64, x64 = out.double().requires_grad_(True), x.double().requires_grad_(True)
    z_ref, ld_ref = _coupling_ref(o64, x64, lens, sig)
    torch.autograd.backward((z_ref, ld_ref), (dz.double(), dld.double()))
    od, xd, dzd, dldd = cuda(out, x, dz, dld)
    od.requires_grad_(True); xd.requires_grad_(True)
    z, ld = glow.coupling(od, xd, i32(lens), sig)
    torch.autograd.backward((z, ld), (dzd, dldd))
    close(z, z_ref.detach(), F32_TOL, "z")
    close(ld, ld_ref.detach(), SUM_TOL if t > 1000 else F32_TOL, "logdet")
    close(od.grad, o64.grad, F32_TOL, "dout")
    close(xd.grad, x64.grad, F32_TOL, "dx")
    back = glow.coupling_reverse(od.detach(), z.detach(), i32(lens), sig)
    h = c // 2
    close(back[..., h:], (x.double() * valid(lens, t))[..., h:], 1e-4, "reverse(forward(x))")   # exp(logs) exp(-logs) in fp32
    assert torch.equal(back[..., :h], xd.detach()[..., :h])
    close(glow.coupling_reverse(od.detach(), xd.detach(), i32(lens), sig), _coupling_ref(out.double(), x.double(), lens, sig, True)[0],
          F32_TOL, "reverse")


# ------------------------------------------------------------------------------------------------ relative attention
def _attn_ref(q, k, v, ek, ev, lens, heads, window, keep=None):
    """AttentionBlock.attention (submodules.py:463-512) on channels-last [B, T, C] through the oracle's rel_to_abs /
    abs_to_rel; any device, any dtype."""
    b, t, c = q.shape
    d = c // heads
    qh, kh, vh = (a.view(b, t, heads, d).transpose(1, 2) for a in (q, k, v))
    scores = qh @ kh.transpose(-2, -1) / math.sqrt(d)
    ekr = go.rel_embeddings(ek.view(1, -1, d), t, window)
    scores = scores + go.rel_to_abs(qh @ ekr.unsqueeze(0).transpose(-2, -1)) / math.sqrt(d)
    ok = torch.arange(t, device=q.device)[None, :] < lens.to(q.device)[:, None]
    mask = (ok[:, None, :, None] & ok[:, None, None, :])
    pa = F.softmax(scores.masked_fill(~mask, -1e4), dim=-1)
    if keep is not None:
        pa = pa * keep.view(b, heads, t, t).to(pa)
    out = pa @ vh + go.abs_to_rel(pa) @ go.rel_embeddings(ev.view(1, -1, d), t, window).unsqueeze(0)
    return out.transpose(1, 2).reshape(b, t, c)


def _attn_case(b, t, heads, d, window, lens, p, seed=8, dev_ref="cpu", tol=SUM_TOL):
    from smt_amd import glow
    g = gen(seed)
    c = heads * d
    # zero-padded rows: a padded query row averages the values of ALL keys in the reference, which the kernel reads as zero
    # beyond lens (test_padding_contract_rel_attention puts garbage and NaN there)
    q, k, v = (torch.randn(b, t, c, generator=g) * valid(lens, t) for _ in range(3))
    ek, ev = (torch.randn(1, 2 * window + 1, d, generator=g) * d ** -0.5 for _ in range(2))
    dctx = torch.randn(b, t, c, generator=g) * valid(lens, t)
    drop = make_drop(p, seed=13, site=1) if p > 0 else make_drop(0.0)
    keep = drop_keep(13, 1, b * heads * t * t, p) if p > 0 else None
    args64 = [a.double().to(dev_ref).requires_grad_(True) for a in (q, k, v, ek, ev)]
    ref = _attn_ref(*args64[:3], args64[3], args64[4], lens, heads, window, keep)
    ref.backward(dctx.double().to(dev_ref))
    argd = [a.to(DEV).requires_grad_(True) for a in (q, k, v, ek, ev)]
    ctx = glow.rel_attention(*argd, i32(lens), heads, window, drop)
    ctx.backward(dctx.to(DEV))
    close(ctx, ref.detach(), F32_TOL if t < 1000 else tol, "ctx")
    for name, got, want in zip(("dq", "dk", "dv", "d emb_rel_k", "d emb_rel_v"), argd, args64):
        close(got.grad, want.grad, tol, name)


ATTN_CASES = [  # b, t, heads, head_dim, window, lens
    (1, 1, 2, 96, 4, [1]),
    (2, 3, 2, 96, 4, [3, 1]),             # t <= W
    (2, 9, 2, 96, 4, [9, 0]),             # t = 2W + 1; an item with no valid position
    (2, 9, 1, 1, 0, [9, 4]),              # head_dim 1, window 0
    (2, 255, 2, 96, 4, [255, 1]),
    (2, 256, 2, 96, 4, [256, 200]),
    (2, 257, 2, 96, 4, [256, 257]),       # the j-loops' 256-key stride, a padded last key
    (1, 513, 2, 96, 0, [500]),
    (3, 200, 2, 96, 4, [200, 137, 1]),    # configs[4]: hidden 192, 2 heads, window 4, T_x ~ 200
]


@pytest.mark.parametrize("b,t,heads,d,window,lens", ATTN_CASES)
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_rel_attention_forward_backward(b, t, heads, d, window, lens, p):
    _attn_case(b, t, heads, d, window, torch.tensor(lens), p)


def test_rel_attention_at_the_lds_limit():
    """The largest t that the 60 KiB LDS check admits (fwd: (head_dim + t) * 4 B, bwd: (2 head_dim + t) * 4 B) computes the
    right thing; one more key is refused by the argument check (RuntimeError from N.check), before any launch.  head_dim 1,
    1 head: the float64 reference ([t, t] scores) runs on the device, the CPU would take minutes."""
    from smt_amd import glow
    t_bwd = 60 * 1024 // 4 - 2
    _attn_case(1, t_bwd, 1, 1, 4, torch.tensor([t_bwd - 5]), 0.0, dev_ref=DEV, tol=1e-3)   # softmax sums over 15k keys
    t_fwd = t_bwd + 1                               # forward admitted, backward refused
    q = torch.randn(1, t_fwd, 1, device=DEV, requires_grad=True)
    e = torch.zeros(1, 9, 1, device=DEV)
    lens = torch.tensor([t_fwd], dtype=torch.int32, device=DEV)
    ctx = glow.rel_attention(q, q.detach(), q.detach(), e, e, lens, 1, 4)
    assert torch.isfinite(ctx).all()
    with pytest.raises(RuntimeError, match="LDS"):
        ctx.backward(torch.ones_like(ctx))
    with pytest.raises(RuntimeError, match="LDS"):
        glow.rel_attention(torch.zeros(1, t_fwd + 1, 1, device=DEV), *(torch.zeros(1, t_fwd + 1, 1, device=DEV),) * 2, e, e,
                           torch.tensor([1], dtype=torch.int32, device=DEV), 1, 4)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ prior log-likelihood
@pytest.mark.parametrize("b,tx,ty,dim", [(1, 1, 1, 80), (2, 17, 300, 80), (2, 200, 870, 160), (1, 3, 257, 1)])
@pytest.mark.parametrize("mean_only", [False, True])
def test_prior_logp(b, tx, ty, dim, mean_only):
    from smt_amd import glow
    g = gen(9)
    xm, z = torch.randn(b, tx, dim, generator=g), torch.randn(b, ty, dim, generator=g)
    xl = None if mean_only else 0.3 * torch.randn(b, tx, dim, generator=g)
    xl64 = torch.zeros(b, tx, dim, dtype=torch.float64) if mean_only else xl.double()
    ref = (-0.5 * math.log(2 * math.pi) - xl64[:, :, None, :]
           - 0.5 * (z.double()[:, None, :, :] - xm.double()[:, :, None, :]) ** 2 * torch.exp(-2 * xl64[:, :, None, :])).sum(-1)
    got = glow.prior_logp(xm.to(DEV), None if mean_only else xl.to(DEV), z.to(DEV))
    close(got, ref, F32_TOL, "logp")


# ------------------------------------------------------------------------------------------------ alignment
def _hand_path(b, tx, ty, durs, y_lens):
    path = torch.zeros(b, tx, ty)
    for i in range(b):
        j = 0
        for tok, n in enumerate(durs[i]):
            path[i, tok, j:j + n] = 1
            j += n
        assert j <= y_lens[i]
    return path


def _check_alignment(path, d=80):
    from smt_amd import glow
    b, tx, ty = path.shape
    idx, dur = glow.align_index(path.to(DEV))
    tok = torch.where(path.any(1), tx - 1 - path.flip(1).argmax(1), torch.full((b, ty), -1))
    assert torch.equal(idx.cpu().long(), tok), "frame -> token index"
    assert torch.equal(dur.cpu(), path.sum(-1)), "durations"
    x = torch.randn(b, tx, d, generator=gen(10))
    dz = torch.randn(b, ty, d, generator=gen(11))
    x64 = x.double().requires_grad_(True)
    ref = path.double().transpose(1, 2) @ x64                   # z_m = x_m @ attn (glow_tts.py:100), channels-last
    ref.backward(dz.double())
    xd = x.to(DEV).requires_grad_(True)
    z = glow.align_gather(xd, idx)
    z.backward(dz.to(DEV))
    close(z, ref.detach(), 0.0, "gather")
    close(xd.grad, x64.grad, F32_TOL, "scatter")


def test_alignment_on_hand_built_paths():
    """Tokens of duration 0, frames beyond y_len (no token), one token only."""
    _check_alignment(_hand_path(3, 5, 20, [[3, 0, 4, 0, 2], [0, 0, 1, 0, 0], [5, 5, 5, 0, 5]], [9, 1, 20]))
    _check_alignment(_hand_path(2, 1, 33, [[33], [7]], [33, 7]))
    _check_alignment(torch.zeros(2, 4, 6))


@pytest.mark.parametrize("b,tx,ty", [(2, 7, 30), (2, 200, 870)])
def test_alignment_on_searched_paths(b, tx, ty):
    from models.glow_tts import submodules as S
    g = gen(12)
    logp = torch.randn(b, tx, ty, generator=g)
    x_lens, y_lens = torch.tensor([tx, max(1, tx // 3)]), torch.tensor([ty, max(tx // 3, ty // 2)])
    mask = (go.sequence_mask(x_lens, tx).unsqueeze(-1) & go.sequence_mask(y_lens, ty).unsqueeze(1)).float()
    path = S.maximum_path(logp.to(DEV), mask.to(DEV)).cpu()
    _check_alignment(path)


# ------------------------------------------------------------------------------------------------ losses
@pytest.mark.parametrize("n_shape", [(1, 1, 1), (2, 37, 80), (2, 435, 160), (3, 2301, 160)])   # 1.1 M elements > 4096 * 256
@pytest.mark.parametrize("with_logs", [True, False])
def test_mle_loss(n_shape, with_logs):
    from smt_amd import glow
    g = gen(13)
    z, zm = torch.randn(*n_shape, generator=g), torch.randn(*n_shape, generator=g)
    zl = 0.3 * torch.randn(*n_shape, generator=g) if with_logs else None
    logdet, denom = torch.tensor(3.5), torch.tensor(float(z.numel()) * 0.8)
    z64, zm64, ld64 = (a.double().requires_grad_(True) for a in (z, zm, logdet))
    zl64 = zl.double().requires_grad_(True) if with_logs else torch.zeros_like(z64)
    ref = 0.5 * math.log(2 * math.pi) + (zl64.sum() + 0.5 * (torch.exp(-2 * zl64) * (z64 - zm64) ** 2).sum() - ld64) / denom.double()
    ref.backward()
    zd, zmd, ldd = (a.to(DEV).requires_grad_(True) for a in (z, zm, logdet))
    zld = zl.to(DEV).requires_grad_(True) if with_logs else None
    loss = glow.mle_loss(zd, zmd, zld, ldd, denom.to(DEV))
    loss.backward()
    close(loss, ref.detach(), SUM_TOL if z.numel() > 100000 else F32_TOL, "loss")     # 4096 partial sums in sequence
    close(zd.grad, z64.grad, F32_TOL, "dz")
    close(zmd.grad, zm64.grad, F32_TOL, "dz_m")
    close(ldd.grad, ld64.grad, F32_TOL, "dlogdet")
    if with_logs:
        close(zld.grad, zl64.grad, F32_TOL, "dz_logs")


def _length_ref(logw, dur, lens, denom):
    m = valid(lens, logw.shape[1]).squeeze(-1).double()
    return (((logw - torch.log(1e-8 + dur) * m) * m) ** 2).sum() / denom


@pytest.mark.parametrize("b,tx,lens", [(1, 1, [1]), (3, 20, [20, 1, 0]), (4, 300, [300, 1, 0, 257]), (2, 1500, [1500, 999])])
def test_length_loss(b, tx, lens):
    """B T_x > 1024 loops the single 1024-thread workgroup."""
    from smt_amd import glow
    g = gen(14)
    logw, dur = torch.randn(b, tx, generator=g), torch.randint(0, 9, (b, tx), generator=g).float()
    lens = torch.tensor(lens)
    denom = torch.tensor(float(max(1, int(lens.sum()))))
    lw64 = logw.double().requires_grad_(True)
    ref = _length_ref(lw64, dur.double(), lens, denom.double())
    ref.backward()
    lwd = logw.to(DEV).requires_grad_(True)
    loss = glow.length_loss(lwd, dur.to(DEV), i32(lens), denom.to(DEV))
    loss.backward()
    close(loss, ref.detach(), F32_TOL, "loss")
    close(lwd.grad, lw64.grad, F32_TOL, "dlogw")


# ------------------------------------------------------------------------------------------------ GlowTTS convolution shapes
CONV_SHAPES = [  # c_in, c_out, k, x channels (> c_in: the layer reads the leading c_in)
    (192, 384, 5, 192),     # WN in_layer
    (192, 768, 3, 192), (768, 192, 3, 768),     # FFN
    (192, 256, 3, 192), (256, 256, 3, 256),     # duration predictor
    (80, 192, 1, 160),      # coupling `start` on x0 = the first 80 of 160 channels: c_use = 128 reads x1's first 48 (zero weights)
    (192, 80, 1, 192),      # proj_m: 80 output channels run as o_use = 128
    (192, 384, 1, 192), (192, 192, 1, 192),     # res/skip projections
]


@pytest.mark.parametrize("cin,cout,k,cx", CONV_SHAPES)
def test_glow_conv_shapes_against_float64(cin, cout, k, cx):
    """fp32 through models/glow_tts/submodules.conv with ragged lens, T = 211 (not a multiple of any tile): forward, data
    gradient and weight / bias gradients against F.conv1d in float64 on the masked input.  The padded rows of x hold
    garbage: the kernels read them as zero."""
    from models.glow_tts import submodules as S
    g = gen(15)
    b, t = 3, 211
    lens = torch.tensor([211, 1, 150])
    x = torch.randn(b, t, cx, generator=g)
    w, bias = torch.randn(cout, cin, k, generator=g) / math.sqrt(cin * k), 0.1 * torch.randn(cout, generator=g)
    dy = torch.randn(b, t, cout, generator=g)
    m = valid(lens, t)
    x64, w64, b64 = (a.double().requires_grad_(True) for a in (x[..., :cin] * m, w, bias))
    ref = F.conv1d(x64.transpose(1, 2), w64, b64, padding=k // 2).transpose(1, 2)
    ref.backward(dy.double())
    xd, wd, bd = (a.to(DEV).requires_grad_(True) for a in (pad_as(x, lens, "garbage"), w, bias))
    y = S.conv(xd, wd, bd, padding=k // 2, lens=i32(lens), x_channels=cin)
    y.backward(dy.to(DEV))
    conv_tol = dict(f=2e-5, g=2e-4)           # as tests/test_conv_gpu.py for fp32: MFMA sums over c_in * k terms
    close(y, ref.detach(), conv_tol["f"], "y")
    close(xd.grad[..., :cin] * m.to(DEV), x64.grad * m, conv_tol["f"], "dx (valid rows)")
    if cx > cin:
        assert not xd.grad[..., cin:].abs().gt(0).any(), "gradient leaked into the channels the layer does not read"
    close(wd.grad, w64.grad, conv_tol["g"], "dW")
    close(bd.grad, b64.grad, conv_tol["g"], "dbias")


# ------------------------------------------------------------------------------------------------ padding contract
def _run_three(fn, inputs, n_rows, lens, grads_at):
    """fn(list of device inputs (requires_grad), lens) -> outputs; runs with the padded rows of the first n_rows inputs (the
    [B, T, C] ones) zero, +-1e3 garbage and NaN.  Returns [(outputs, input grads)] for the three fills."""
    res = []
    for fill in (0.0, "garbage", float("nan")):
        xs = [(pad_as(a, lens, fill) if n < n_rows else a).to(DEV).requires_grad_(True) for n, a in enumerate(inputs)]
        outs = fn(xs, i32(lens))
        torch.autograd.backward([o for o in outs if o.requires_grad], [gr.to(DEV) for gr, o in zip(grads_at, outs) if o.requires_grad])
        res.append(([o.detach() for o in outs], [a.grad for a in xs]))
    return res


def _assert_contract(res, lens, out_rowwise, grad_rowwise, what):
    """Rowwise tensors: valid rows must be bit-identical to the zero-padded run (garbage AND NaN); reductions / parameter
    gradients: bit-identical.  With finite garbage, the zero-padded run's padded rows are reproduced where the op zeroes them."""
    (o0, g0) = res[0]
    for run, fill in ((res[1], "garbage"), (res[2], "NaN")):
        o, gr = run
        for kind, a_list, b_list, rowwise in (("out", o, o0, out_rowwise), ("grad", gr, g0, grad_rowwise)):
            for i, (a, b) in enumerate(zip(a_list, b_list)):
                if rowwise[i] is None:
                    continue
                if rowwise[i]:
                    m = valid(lens, a.shape[1]).to(DEV).expand_as(a)
                    bits_equal(a[m], b[m], f"{what} {kind}[{i}] valid rows ({fill} padding)")
                else:
                    bits_equal(a, b, f"{what} {kind}[{i}] ({fill} padding)")


def test_padding_contract_actnorm_invconv_coupling():
    from smt_amd import glow
    b, t, c = 3, 200, 160
    lens = torch.tensor([200, 1, 133])
    g = gen(16)
    x, out = torch.randn(b, t, c, generator=g), torch.randn(b, t, c, generator=g)
    dz = torch.randn(b, t, c, generator=g) * valid(lens, t)
    logs, bias, w = 0.3 * torch.randn(c, generator=g), torch.randn(c, generator=g), torch.linalg.qr(torch.randn(4, 4, generator=g))[0]
    dld = torch.randn(b, generator=g)
    res = _run_three(lambda xs, l: [glow.actnorm(xs[0], xs[1], xs[2], l)], [x, logs, bias], 1, lens, [dz])
    _assert_contract(res, lens, [True], [True, False, False], "actnorm")
    for r in res:                             # padded rows of z and dx are zero whatever the input held
        pad = ~valid(lens, t).to(DEV).expand(b, t, c)
        assert not r[0][0][pad].any() and not r[1][0][pad].any()
    res = _run_three(lambda xs, l: [glow.invconv(xs[0], xs[1], l)], [x, w], 1, lens, [dz])
    _assert_contract(res, lens, [True], [True, False], "invconv")
    for sig in (False, True):
        res = _run_three(lambda xs, l: list(glow.coupling(xs[0], xs[1], l, sig)), [out, x], 2, lens, [dz, dld])
        _assert_contract(res, lens, [True, False], [True, True], f"coupling(sigmoid_scale={sig})")
    xn = pad_as(x, lens, float("nan")).to(DEV)
    cnt, s1, s2 = glow.masked_channel_moments(xn, i32(lens))
    assert torch.isfinite(torch.stack([cnt, s1, s2])).all()
    for fn, args in ((glow.actnorm_reverse, (xn, logs.to(DEV), bias.to(DEV))), (glow.invconv_reverse, (xn, w.to(DEV)))):
        zr = fn(*args, i32(lens))
        assert torch.isfinite(zr).all(), fn.__name__       # padded rows of the reverse flows are zero, not NaN
    zr = glow.coupling_reverse(pad_as(out, lens, float("nan")).to(DEV), xn, i32(lens))
    assert torch.isfinite(zr[..., c // 2:]).all()


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_padding_contract_rel_attention(p):
    """Padded rows of q, k, v hold garbage / NaN; the upstream gradient is zero there (the next op masks it).  ctx at valid
    rows, every gradient at valid rows and both relative-embedding gradients are bit-identical to the zero-padded run; with
    zero padding the padded query rows match the reference (uniform over all T keys)."""
    from smt_amd import glow
    b, t, heads, d, window = 3, 257, 2, 96, 4
    lens = torch.tensor([257, 1, 130])
    g = gen(17)
    q, k, v = (torch.randn(b, t, heads * d, generator=g) for _ in range(3))
    ek, ev = (torch.randn(1, 2 * window + 1, d, generator=g) * d ** -0.5 for _ in range(2))
    dctx = torch.randn(b, t, heads * d, generator=g) * valid(lens, t)
    drop = make_drop(p, seed=21, site=2) if p > 0 else make_drop(0.0)
    res = _run_three(lambda xs, l: [glow.rel_attention(*xs, l, heads, window, drop)], [q, k, v, ek, ev], 3, lens, [dctx])
    _assert_contract(res, lens, [True], [True, True, True, False, False], "rel_attention")
    keep = drop_keep(21, 2, b * heads * t * t, p) if p > 0 else None
    ref = _attn_ref(*(a.double() * valid(lens, t) for a in (q, k, v)), ek.double(), ev.double(), lens, heads, window, keep)
    close(res[0][0][0], ref, F32_TOL, "ctx, padded query rows included")


def test_padding_contract_length_loss():
    from smt_amd import glow
    b, tx = 4, 300
    lens = torch.tensor([300, 1, 0, 257])
    g = gen(18)
    logw, dur = torch.randn(b, tx, generator=g), torch.randint(0, 9, (b, tx), generator=g).float()
    runs = []
    for fill in (0.0, "garbage", float("nan")):
        lw = pad_as(logw.unsqueeze(-1), lens, fill).squeeze(-1).to(DEV).requires_grad_(True)
        du = pad_as(dur.unsqueeze(-1), lens, fill).squeeze(-1).abs().to(DEV)
        loss = glow.length_loss(lw, du, i32(lens), torch.tensor(float(lens.sum()), device=DEV))
        loss.backward()
        runs.append((loss.detach(), lw.grad))
    for loss, grad in runs[1:]:
        bits_equal(loss.reshape(1), runs[0][0].reshape(1), "length loss")
        bits_equal(grad, runs[0][1], "dlogw")       # padded entries: exactly 0


# ------------------------------------------------------------------------------------------------ one full-width model
def test_full_width_glow_tts_matches_float64_oracle(monkeypatch):
    """configs/models/glow_tts.yaml as it stands (hidden 192, filter 768, 6 encoder layers, 12 flow blocks of 4 WN layers, 80
    mels -> 160 flow channels), dropout 0, B = 2, ragged T_x ~ 150 / T_y ~ 800, against go.glow_tts_forward in float64; the
    CPU oracle's forward + backward takes about a second on 16 threads (printed).  Both sides use the product's alignment:
    at this size fp32 and float64 log-likelihoods can flip a near-tie of the search, which would move the duration loss by
    far more than any kernel error; the search itself is checked against the oracle's own (at most 1% of frames differ, and
    tests/test_mas_gpu.py pins it exactly).  Losses 1e-5; z and logdet by max-abs relative to their max; every parameter
    gradient by the per-tensor relative L2 of test_train_mode_with_dropout_matches_the_oracle (5e-3) plus a max-abs bound
    relative to the tensor's max (2e-2: 36 fp32 flow steps and 6 attention layers of MFMA sums)."""
    import os
    import time
    from models.glow_tts.glow_tts import GlowTTS
    from utils import config as C
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "speech-masters-thesis_amd")
    m = C.load(os.path.join(pkg, "configs/models/glow_tts.yaml")).model
    enc = {k: m.encoder[k] for k in ("n_vocab", "hidden_channels", "filter_channels", "kernel_size", "n_layers", "n_heads", "window_size",
                                      "prenet", "mean_only")}
    enc.update(filter_channels_dp=m.encoder.filter_channels, p_dropout=0.0)
    dec = {k: m.decoder[k] for k in ("hidden_channels", "kernel_size", "n_layers", "n_sqz", "n_split", "sigmoid_scale", "dilation_rate")}
    dec.update(p_dropout=0.0, n_blocks=m.decoder.n_blocks)
    assert enc["hidden_channels"] == 192 and enc["filter_channels"] == 768 and enc["n_layers"] == 6
    assert dec["n_blocks"] == 12 and dec["n_layers"] == 4
    cfg = dict(encoder=enc, decoder=dec, zero_out=False)
    n_vocab, n_mels = enc["n_vocab"], 80
    p32 = go.init_params(cfg, n_vocab, n_mels, seed=31)
    model = GlowTTS(C.create({"model": dict(n_speakers=1, gin_channels=0, encoder=dict(enc), decoder=dict(dec)),
                              "dataset": dict(n_mels=n_mels, intersperse_blanks=False, cmudict_path="")})).to(DEV)
    model.load_state_dict({k: v.float() for k, v in p32.items()}, strict=True)
    model.encoder.pre.p_dropout = 0.0
    tokens, x_lens, y, y_lens = go.synthetic_batch(2, 150, 800, n_vocab, n_mels, seed=32)
    from models.glow_tts import submodules as S
    paths, search = [], S.maximum_path

    def product_search(value, mask, *a):
        paths.append(search(value, mask, *a))
        return paths[-1]
    monkeypatch.setattr(S, "maximum_path", product_search)
    own = []
    oracle_search = go.mas_oracle.maximum_path

    def replay(value, mask, *a):
        own.append(oracle_search(value, mask, *a))
        return paths[-1].cpu().numpy().astype(own[-1].dtype)
    monkeypatch.setattr(go.mas_oracle, "maximum_path", replay)
    model.train()
    loss_dict, _ = model(tokens.to(DEV), x_lens.to(DEV), y.to(DEV), y_lens.to(DEV))
    loss_dict["loss"].backward()
    p64 = {k: v.double().requires_grad_(True) for k, v in p32.items()}
    t0 = time.time()
    out, aux = go.glow_tts_forward(tokens, x_lens, y.double(), y_lens, p64, cfg, True)
    out["loss"].backward()
    flips = int((own[0].argmax(1) != paths[0].cpu().numpy().argmax(1)).sum())
    print(f"\n[full-width glow_tts] float64 CPU oracle forward + backward: {time.time() - t0:.1f} s; "
          f"{flips} of {int(y_lens.sum()) // 2 * 2} frames aligned differently by the oracle's own search")
    assert flips <= 0.01 * int(y_lens.sum())
    assert np.isclose(loss_dict["loss_mle"].item(), float(out["loss_mle"]), rtol=1e-5, atol=0)
    assert np.isclose(loss_dict["loss_length"].item(), float(out["loss_length"]), rtol=1e-5, atol=0)
    with torch.no_grad():                       # z and logdet of the product's flow on the same frames
        yl = ((y_lens // 2) * 2).to(torch.int32).to(DEV)
        spect = y.to(DEV)[:, :, :(y.shape[2] // 2) * 2].transpose(1, 2).contiguous()
        z, logdet = model.decoder(spect, yl, reverse=False)
    mz = valid(yl.cpu(), z.shape[1]).to(DEV)
    close(z * mz, aux["z_dec"].transpose(1, 2) * mz.cpu(), 1e-4, "z")        # 36 fp32 flow steps of MFMA convolutions
    close(logdet, aux["logdet"], SUM_TOL, "logdet")                           # sums of ~30,000 coupling log-scales per flow
    worst = (0.0, "")
    gmax = max(float(v.grad.norm()) for v in p64.values())
    for name, prm in model.named_parameters():
        ref = p64[name].grad
        e = float((prm.grad.double().cpu() - ref).norm() / (ref.norm() + 1e-6 * gmax))
        a = float((prm.grad.double().cpu() - ref).abs().max() / (ref.abs().max() + 1e-6 * gmax))
        worst = max(worst, (max(e, a / 4), name))
        assert e <= 5e-3 and a <= 2e-2, (name, e, a)
    print(f"  worst gradient error {worst}")
