"""The bf16 projections of the TransformerLM (csrc/lm_linear.hip: smt_lm_linear_fwd / _dgrad / _wgrad, and smt_amd.lm.linear on
top of them) against the float64 evaluation and the derived bound of tests/lm_linear_helpers.py.  Exact integer data first:
that is what catches a permuted operand map."""
import ctypes
import functools

import pytest
import torch

import lm_linear_helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def _p(t, offset_elems=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + 4 * offset_elems)


def _packed(w):
    """(w_packed [n_out][n_in], w_packed_t [n_in][n_out]) through the library's own pack kernels."""
    from smt_amd import lm as K
    wp, wt = K._packed_bf16(w, False), K._packed_bf16(w, True)
    assert torch.equal(wp[0], w.to(torch.bfloat16)) and torch.equal(wt[0], w.to(torch.bfloat16).T)   # torch's rounding, bit for bit
    return wp, wt


def raw_fwd(x, ld_x, wp, bias, y, ld_y, rows, n_in, n_out):
    from smt_amd import native as N
    N.check(N.lib().smt_lm_linear_fwd(_p(x), ld_x, _p(wp), _p(bias), _p(y), ld_y, rows, n_in, n_out, N.stream_ptr()), "smt_lm_linear_fwd")


def raw_dgrad(dy, ld_dy, wt, dx, ld_dx, rows, n_in, n_out):
    from smt_amd import native as N
    N.check(N.lib().smt_lm_linear_dgrad(_p(dy), ld_dy, _p(wt), _p(dx), ld_dx, rows, n_in, n_out, N.stream_ptr()), "smt_lm_linear_dgrad")


def raw_wgrad(x, ld_x, dy, ld_dy, dw, db, rows, n_in, n_out, ws="auto"):
    from smt_amd import native as N
    if ws == "auto":
        nbytes = N.lib().smt_lm_linear_wgrad_workspace_bytes(rows, n_in, n_out)
        ws = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=DEV)
    N.check(N.lib().smt_lm_linear_wgrad(_p(x), ld_x, _p(dy), ld_dy, _p(dw), _p(db), rows, n_in, n_out, _p(ws),
                                        0 if ws is None else ws.numel(), N.stream_ptr()), "smt_lm_linear_wgrad")


def run_all(x, w, bias, dy, with_bias=True):
    """(y, dx, dw, db) of the three entries on dense operands."""
    rows, n_in = x.shape
    n_out = w.shape[0]
    wp, wt = _packed(w)
    y = torch.full((rows, n_out), NAN, device=DEV)
    dx = torch.full((rows, n_in), NAN, device=DEV)
    dw = torch.full((n_out, n_in), NAN, device=DEV)
    db = torch.full((n_out,), NAN, device=DEV) if with_bias else None
    raw_fwd(x, n_in, wp, bias if with_bias else None, y, n_out, rows, n_in, n_out)
    raw_dgrad(dy, n_out, wt, dx, n_in, rows, n_in, n_out)
    raw_wgrad(x, n_in, dy, n_out, dw, db, rows, n_in, n_out)
    return y, dx, dw, db


@functools.lru_cache(maxsize=None)
def reference(rows, n_in, n_out):
    """The case and its float64 references on the device, computed once per shape; callers leave them alone."""
    x, w, bias, dy = H.make_case(rows, n_in, n_out, DEV)
    return dict(x=x, w=w, bias=bias, dy=dy, y=H.fwd_ref(x, w, bias), y_nobias=H.fwd_ref(x, w), dx=H.dgrad_ref(dy, w),
                wg=H.wgrad_ref(x, dy))


def check_all(tag, got, ref, with_bias=True):
    y, dx, dw, db = got
    H.check(f"{tag} fwd", y, *ref["y" if with_bias else "y_nobias"])
    H.check(f"{tag} dgrad", dx, *ref["dx"])
    dw_ref, dw_b, db_ref, db_b = ref["wg"]
    H.check(f"{tag} wgrad", dw, dw_ref, dw_b)
    if with_bias:
        H.check(f"{tag} dbias", db, db_ref, db_b)


@pytest.mark.parametrize("rows,n_in,n_out", H.EXACT_SHAPES)
def test_exact_integer_data_gives_the_exact_result(rows, n_in, n_out):
    x, w, bias, dy = H.make_exact_case(rows, n_in, n_out, DEV)
    y, dx, dw, db = run_all(x, w, bias, dy)
    assert torch.equal(y.double(), x.double() @ w.double().T + bias.double())
    assert torch.equal(dx.double(), dy.double() @ w.double())
    assert torch.equal(dw.double(), dy.double().T @ x.double())
    assert torch.equal(db.double(), dy.double().sum(0))


@pytest.mark.parametrize("n_in,n_out", H.SMALL_DIMS)
@pytest.mark.parametrize("rows", H.SMALL_ROWS)
def test_small_shapes_stay_inside_the_float64_bound(rows, n_in, n_out):
    ref = reference(rows, n_in, n_out)
    check_all(f"({rows}, {n_in}, {n_out})", run_all(ref["x"], ref["w"], ref["bias"], ref["dy"]), ref)


@pytest.mark.parametrize("rows,n_in,n_out", H.WIDE_SHAPES + [H.PRODUCT_SHAPE])
def test_model_widths_stay_inside_the_float64_bound(rows, n_in, n_out):
    ref = reference(rows, n_in, n_out)
    check_all(f"({rows}, {n_in}, {n_out})", run_all(ref["x"], ref["w"], ref["bias"], ref["dy"]), ref)


def test_without_bias_and_without_dbias():
    ref = reference(129, 64, 192)
    got = run_all(ref["x"], ref["w"], ref["bias"], ref["dy"], with_bias=False)
    assert got[3] is None
    check_all("no bias", got, ref, with_bias=False)


def test_column_slices_of_wider_tensors_are_read_and_written_in_place():
    """x, y, dy and dx as column slices (pitch > width) of tensors whose other columns hold NaN: a read outside the slice
    poisons the result, a write outside it removes a NaN."""
    rows, n_in, n_out = 129, 64, 192
    ref = reference(rows, n_in, n_out)
    wp, wt = _packed(ref["w"])

    def wide(t, left, right):
        out = torch.full((rows, left + t.shape[1] + right), NAN, device=DEV)
        out[:, left:left + t.shape[1]] = t
        return out, left

    def untouched(buf, left, width):
        return bool(torch.isnan(buf[:, :left]).all()) and bool(torch.isnan(buf[:, left + width:]).all())

    xw, xo = wide(ref["x"], 8, 4)
    dyw, dyo = wide(ref["dy"], 4, 12)
    yw, yo = wide(torch.zeros(rows, n_out, device=DEV), 12, 8)
    dxw, dxo = wide(torch.zeros(rows, n_in, device=DEV), 4, 4)
    dw = torch.empty(n_out, n_in, device=DEV)
    db = torch.empty(n_out, device=DEV)
    from smt_amd import native as N
    lib = N.lib()
    N.check(lib.smt_lm_linear_fwd(_p(xw, xo), xw.shape[1], _p(wp), _p(ref["bias"]), _p(yw, yo), yw.shape[1], rows, n_in, n_out,
                                  N.stream_ptr()), "fwd")
    N.check(lib.smt_lm_linear_dgrad(_p(dyw, dyo), dyw.shape[1], _p(wt), _p(dxw, dxo), dxw.shape[1], rows, n_in, n_out, N.stream_ptr()),
            "dgrad")
    ws = torch.empty(max(int(lib.smt_lm_linear_wgrad_workspace_bytes(rows, n_in, n_out)), 16), dtype=torch.uint8, device=DEV)
    N.check(lib.smt_lm_linear_wgrad(_p(xw, xo), xw.shape[1], _p(dyw, dyo), dyw.shape[1], _p(dw), _p(db), rows, n_in, n_out, _p(ws),
                                    ws.numel(), N.stream_ptr()), "wgrad")
    assert untouched(yw, yo, n_out) and untouched(dxw, dxo, n_in)
    check_all("pitched", (yw[:, yo:yo + n_out], dxw[:, dxo:dxo + n_in], dw, db), ref)
    # the autograd op takes the same slices without copying them
    from smt_amd import lm as K
    xs = xw[:, xo:xo + n_in]
    assert K._rows(xs, n_in)[0] is xs and K._rows(xs, n_in)[1] == xw.shape[1]
    H.check("pitched K.linear", K.linear(xs, ref["w"], ref["bias"], compute_dtype=torch.bfloat16), *ref["y"])


def test_equal_inputs_give_equal_bits():
    ref = reference(*H.WIDE_SHAPES[0])
    a = run_all(ref["x"], ref["w"], ref["bias"], ref["dy"])
    b = run_all(ref["x"], ref["w"], ref["bias"], ref["dy"])
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_zero_rows():
    n_in, n_out = 64, 48
    _, w, bias, _ = H.make_case(1, n_in, n_out, DEV)
    wp, wt = _packed(w)
    e_in, e_out = torch.full((4, n_in), NAN, device=DEV), torch.full((4, n_out), NAN, device=DEV)      # never read
    guard = torch.full((4, n_out), NAN, device=DEV)                 # rows = 0: nothing may be written
    raw_fwd(e_in, n_in, wp, bias, guard, n_out, 0, n_in, n_out)
    assert bool(torch.isnan(guard).all())
    guard_x = torch.full((4, n_in), NAN, device=DEV)
    raw_dgrad(e_out, n_out, wt, guard_x, n_in, 0, n_in, n_out)
    assert bool(torch.isnan(guard_x).all())
    dw, db = torch.full((n_out, n_in), NAN, device=DEV), torch.full((n_out,), NAN, device=DEV)
    raw_wgrad(e_in, n_in, e_out, n_out, dw, db, 0, n_in, n_out, ws=None)
    assert float(dw.abs().sum()) == 0.0 and float(db.abs().sum()) == 0.0       # the sum over nothing
    from smt_amd import lm as K
    from smt_amd import native as N
    assert N.lib().smt_lm_linear_wgrad_workspace_bytes(0, n_in, n_out) == 0
    xg = torch.empty(2, 0, n_in, device=DEV, requires_grad=True)
    wg = w.clone().requires_grad_(True)
    y = K.linear(xg, wg, bias, compute_dtype=torch.bfloat16)
    assert y.shape == (2, 0, n_out)
    y.sum().backward()
    assert xg.grad.shape == (2, 0, n_in) and float(wg.grad.abs().sum()) == 0.0


def test_argument_errors_are_named_before_any_launch():
    rows, n_in, n_out = 8, 64, 48
    x, w, bias, dy = H.make_case(rows, n_in, n_out, DEV)
    wp, wt = _packed(w)
    y, dx = torch.empty(rows, n_out, device=DEV), torch.empty(rows, n_in, device=DEV)
    dw, db = torch.empty(n_out, n_in, device=DEV), torch.empty(n_out, device=DEV)
    from smt_amd import native as N
    lib, st = N.lib(), N.stream_ptr()

    def fwd(x_=_p(x), ld_x=n_in, wp_=_p(wp), y_=_p(y), ld_y=n_out, rows_=rows, n_in_=n_in, n_out_=n_out):
        N.check(lib.smt_lm_linear_fwd(x_, ld_x, wp_, _p(bias), y_, ld_y, rows_, n_in_, n_out_, st), "smt_lm_linear_fwd")

    def dgrad(dy_=_p(dy), ld_dy=n_out, dx_=_p(dx), ld_dx=n_in, rows_=rows, n_in_=n_in, n_out_=n_out):
        N.check(lib.smt_lm_linear_dgrad(dy_, ld_dy, _p(wt), dx_, ld_dx, rows_, n_in_, n_out_, st), "smt_lm_linear_dgrad")

    def wgrad(x_=_p(x), dy_=_p(dy), dw_=_p(dw), db_=_p(db), ws=None, ws_bytes=0, rows_=rows, n_in_=n_in, n_out_=n_out):
        N.check(lib.smt_lm_linear_wgrad(x_, n_in, dy_, n_out, dw_, db_, rows_, n_in_, n_out_, ws, ws_bytes, st), "smt_lm_linear_wgrad")

    cases = [
        (lambda: fwd(n_in_=48), "n_in=48 must be a positive multiple of 32"),
        (lambda: fwd(n_out_=24), "n_out=24 must be a positive multiple of 16"),
        (lambda: dgrad(n_in_=0), "n_in=0 must be a positive multiple of 32"),
        (lambda: wgrad(n_out_=8), "n_out=8 must be a positive multiple of 16"),
        (lambda: fwd(rows_=-1), "rows=-1 must not be negative"),
        (lambda: wgrad(rows_=-3), "rows=-3 must not be negative"),
        (lambda: fwd(x_=None), r"null pointer \(x\)"),
        (lambda: fwd(wp_=None), r"null pointer \(w_packed\)"),
        (lambda: dgrad(dx_=None), r"null pointer \(dx\)"),
        (lambda: wgrad(dw_=None), r"null pointer \(dweight\)"),
        (lambda: fwd(x_=_p(x, 1)), "x must be 16-byte aligned"),
        (lambda: dgrad(dx_=_p(dx, 2)), "dx must be 16-byte aligned"),
        (lambda: fwd(ld_x=n_in - 4), "pitch ld_x=60 is smaller than the row width 64"),
        (lambda: fwd(ld_y=n_out + 2), "pitch ld_y=50 must be a multiple of 4 elements"),
        (lambda: dgrad(ld_dy=n_out - 16), "pitch ld_dy=32 is smaller than the row width 48"),
        (lambda: fwd(y_=_p(x), ld_y=n_in), "y must not alias x"),
        (lambda: dgrad(dx_=_p(dy, 16), ld_dx=n_in), "dx must not alias dy"),
        (lambda: wgrad(dw_=_p(x)), "dweight must not alias x"),
        (lambda: wgrad(db_=_p(dy)), "dbias must not alias dy"),
    ]
    for call, message in cases:
        with pytest.raises(RuntimeError, match=message):
            call()
    # a row count that needs slabs, and a workspace one byte short of them
    big = 300
    xb, _, _, dyb = H.make_case(big, n_in, n_out, DEV)
    need = lib.smt_lm_linear_wgrad_workspace_bytes(big, n_in, n_out)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="workspace of"):
        wgrad(x_=_p(xb), dy_=_p(dyb), ws=_p(ws), ws_bytes=need - 1, rows_=big)
    with pytest.raises(RuntimeError, match=r"null pointer \(workspace\)"):
        wgrad(x_=_p(xb), dy_=_p(dyb), ws=None, ws_bytes=need, rows_=big)


def test_autograd_op_matches_autograd_on_the_float64_evaluation():
    """K.linear in bf16 with leading shape [3, 43]: y, dx, dweight and dbias inside the bounds; the backward keeps x and the
    weight and nothing else."""
    from smt_amd import lm as K
    n_in, n_out = 64, 192
    x, w, bias, dy = H.make_case(3 * 43, n_in, n_out, DEV)
    xg = x.reshape(3, 43, n_in).clone().requires_grad_(True)
    wg, bg = w.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    y = K.linear(xg, wg, bg, compute_dtype=torch.bfloat16)
    assert y.shape == (3, 43, n_out) and y.dtype == torch.float32
    saved = y.grad_fn.saved_tensors
    assert len(saved) == 2 and saved[0].data_ptr() == xg.data_ptr() and saved[1].data_ptr() == wg.data_ptr()
    y.backward(dy.reshape(3, 43, n_out))
    H.check("autograd y", y.detach().reshape(-1, n_out), *H.fwd_ref(x, w, bias))
    H.check("autograd dx", xg.grad.reshape(-1, n_in), *H.dgrad_ref(dy, w))
    dw_ref, dw_b, db_ref, db_b = H.wgrad_ref(x, dy)
    H.check("autograd dweight", wg.grad, dw_ref, dw_b)
    H.check("autograd dbias", bg.grad, db_ref, db_b)
    # without a bias, and with a weight that needs no gradient
    y2 = K.linear(xg, w, compute_dtype=torch.bfloat16)
    H.check("autograd y, no bias", y2.detach().reshape(-1, n_out), *H.fwd_ref(x, w))
