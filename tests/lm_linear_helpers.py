"""Shared by the tests of the TransformerLM's bf16 projections (csrc/lm_linear.hip behind smt_amd.lm.linear): the float64
evaluation of what the three entries compute from the operands they are handed, and the per-element error bound of their
arithmetic against it.  tests/test_lm_linear_cpu.py pins the evaluation to torch.nn.functional.linear in float64 and shows that
the bound has teeth.

What the entries compute (include/smt_hip.h), with bf16(.) = round to nearest even, which is tensor.to(torch.bfloat16):

    y[r, o]  = bias[o] + sum_i bf16(x[r, i]) * bf16(w[o, i])                       n = n_in
    dx[r, i] = sum_o bf16(dy[r, o]) * bf16(w[o, i])                                n = n_out
    dW[o, i] = sum_r bf16(dy[r, o]) * bf16(x[r, i])                                n = rows
    db[o]    = sum_r dy[r, o]                        from the UNROUNDED dy, in fp32

The bound, derived, not tuned.  The product of two bf16 numbers has 16 significant bits and is exact in fp32, so the only
errors are those of the fp32 additions: n - 1 between the products, one for the bias.  Whatever the order of the additions
(a chain, a tree, partial sums over row splits that are added afterwards), every intermediate sum is at most
mag = |bias| + sum |bf16(a)| |bf16(b)| in magnitude, and one fp32 addition is off by at most 2^-23 of its result when the
adder truncates and 2^-24 when it rounds to nearest.  n additions therefore stay within

    |y - y64| <= (n + 1) * 2^-23 * mag

to first order, and the second-order terms ((n * 2^-23)^2 mag, below 1e-3 of the bound up to n = 8192) fit in the +1.  Because no
order of summation is assumed the same bound covers the split weight gradient.  The tests allow SLACK = 2 times the bound, as
tests/conv_ref_helpers.py does.  db gets rows * 2^-23 * sum_r |dy[r, o]| by the same argument (rows - 1 additions).
An operand map that is permuted, a dropped k-slice or a dropped bias move an element by about |y| itself, thousands of
times the bound; an operand truncated instead of rounded moves it by about 2^-9 sqrt(n) |a||b|, tens of times the bound.
"""
import torch

F32_STEP = 2.0 ** -23
SLACK = 2.0

# (rows, n_in, n_out) of the float64-bound tests: every row residue of the 64- and 128-row tiles, one and several column
# tiles, n_out = 16 (the narrowest), the widest sums of the model, and one shape of the shipped configuration
SMALL_ROWS = [1, 33, 129, 300]
SMALL_DIMS = [(32, 16), (64, 192), (128, 64)]
WIDE_SHAPES = [(300, 512, 1536), (300, 2048, 512)]
PRODUCT_SHAPE = (2064, 512, 2048)
EXACT_SHAPES = [(33, 64, 48), (129, 128, 16)]


def bf16(t):
    """The operand as the kernels see it: fp32 -> bf16 (round to nearest even), as float64."""
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def make_case(rows, n_in, n_out, device="cpu", seed=None):
    """(x [rows, n_in], w [n_out, n_in], bias [n_out], dy [rows, n_out]) fp32, standard normal (w scaled to keep y at O(1))."""
    g = torch.Generator().manual_seed(1 + (rows * 4099 + n_in * 31 + n_out if seed is None else seed))
    x = torch.randn(rows, n_in, generator=g)
    w = torch.randn(n_out, n_in, generator=g) * n_in ** -0.5
    bias = torch.randn(n_out, generator=g)
    dy = torch.randn(rows, n_out, generator=g)
    return tuple(t.to(device) for t in (x, w, bias, dy))


def make_exact_case(rows, n_in, n_out, device="cpu"):
    """The same four tensors with integer values in [-4, 4]: exact in bf16, every sum an integer below 2^24."""
    g = torch.Generator().manual_seed(7 + rows + n_in + n_out)

    def ints(*shape):
        return torch.randint(-4, 5, shape, generator=g).to(torch.float32).to(device)

    return ints(rows, n_in), ints(n_out, n_in), ints(n_out), ints(rows, n_out)


def bound(n, mag):
    return (n + 1) * F32_STEP * mag


def fwd_ref(x, w, bias=None):
    """(y, bound) in float64; x [..., n_in], w [n_out, n_in], bias [n_out] or None."""
    xb, wb = bf16(x), bf16(w)
    y, mag = xb @ wb.T, xb.abs() @ wb.abs().T
    if bias is not None:
        y, mag = y + bias.double(), mag + bias.double().abs()
    return y, bound(w.shape[1], mag)


def dgrad_ref(dy, w):
    """(dx, bound) in float64."""
    db_, wb = bf16(dy), bf16(w)
    return db_ @ wb, bound(w.shape[0], db_.abs() @ wb.abs())


def wgrad_ref(x, dy):
    """(dW, bound, db, bound) in float64; x [rows, n_in], dy [rows, n_out]."""
    xb, dyb = bf16(x), bf16(dy)
    rows = x.shape[0]
    d64 = dy.double()
    return dyb.T @ xb, bound(rows, dyb.abs().T @ xb.abs()), d64.sum(0), rows * F32_STEP * d64.abs().sum(0)


def worst(got, ref, bnd):
    """max over elements of |got - ref| / bound, with 0 / 0 = 0 and x / 0 = inf: <= SLACK passes."""
    err = (got.double() - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bnd)
    return float(ratio.max()) if ratio.numel() else 0.0


def fraction_outside(got, ref, bnd):
    """Fraction of the elements that miss SLACK times the bound (the teeth tests)."""
    return float(((got.double() - ref).abs() > SLACK * bnd).double().mean())


def check(name, got, ref, bnd):
    """Print the figure, then assert it."""
    w = worst(got, ref, bnd)
    print(f"  {name}: worst |err| / bound = {w:.3f} (allowed {SLACK})")
    assert w <= SLACK, f"{name}: |err| / bound = {w:.3f} > {SLACK}"
