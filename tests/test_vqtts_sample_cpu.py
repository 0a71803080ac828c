"""Sampling in the VQTTS code head without a GPU: the entry point is declared, bound and exported under the unchanged ABI
number; its argument errors are decided on the host; the float64 restatement of the noise (tests/vqtts_sample_helpers.py) has
the stated form and draws from softmax(l / T); ``VQTTS.infer`` and ``scripts.synthesize`` refuse bad sampling arguments
before they touch a device."""
import os
import re

import numpy as np
import pytest
import torch

import vqtts_model_helpers as H
import vqtts_sample_helpers as S
from conftest import PKG, REPO

NAME = "smt_vqtts_code_head_sample"
INF = float("inf")


def test_entry_point_is_declared_bound_and_exported():
    from smt_amd import native
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "smt_hip.h")).read(), flags=re.S)
    assert NAME in set(re.findall(r"\b(smt_\w+)\s*\(", header)) and NAME in native.exported_symbols()
    abi = int(re.search(r"smt_abi_version\(void\)\s*\{\s*return\s+(\d+)", open(os.path.join(PKG, "csrc", "common.hip")).read()).group(1))
    lib = native.lib()
    assert abi == native.ABI_VERSION == lib.smt_abi_version() == 10
    res, args = native._SIGNATURES[NAME]
    assert res is native.c_int and len(args) == 14
    assert args[5:11] == [native.c_i64, native.c_int, native.c_int, native.c_int, native.c_f32, native.c_f32]
    # the header's noise constants are the helper's
    text = open(os.path.join(REPO, "include", "smt_hip.h")).read()
    assert f"0x{S.NOISE_ROW:08X}" in text and f"0x{S.NOISE_BIN:08X}" in text
    src = open(os.path.join(PKG, "csrc", "vqtts_codes.hip")).read()
    assert f"CH_NOISE_ROW = 0x{S.NOISE_ROW:08X}u" in src and f"CH_NOISE_BIN = 0x{S.NOISE_BIN:08X}u" in src
    assert S.NOISE_BIN % 2 == 1


def test_argument_errors_need_no_launch():
    from smt_amd import native
    lib = native.lib()
    p = native.c_ptr(4096)                                     # never dereferenced: every call below returns before a launch

    def call(rows=64, t_q=8, c=128, v=512, inv_t=1.0, cut=-INF, h=p, ws=p, ws_bytes=8 * 512 * 128, bias=p, seeds=p, pred=p):
        return lib.smt_vqtts_code_head_sample(h, ws, ws_bytes, bias, seeds, rows, t_q, c, v, inv_t, cut, pred, None, None)

    for kwargs, words in ((dict(c=24), b"channels=24 must be a multiple of 16 up to 256"), (dict(c=272), b"channels=272"),
                          (dict(v=48), b"bins=48 must be a multiple of 32 up to 1024"), (dict(v=1056), b"bins=1056"),
                          (dict(rows=-1), b"rows=-1"), (dict(rows=2 ** 31), b"2^31 - 1"),
                          (dict(t_q=0), b"t_q=0 must be at least 1"), (dict(t_q=-3), b"t_q=-3"),
                          (dict(rows=65), b"rows=65 must be a multiple of t_q=8"),
                          (dict(inv_t=0.0), b"inv_temperature"), (dict(inv_t=-1.0), b"inv_temperature"),
                          (dict(inv_t=INF), b"inv_temperature"), (dict(inv_t=float("nan")), b"inv_temperature"),
                          (dict(cut=0.5), b"cut=0.5 must be <= 0"), (dict(cut=float("nan")), b"cut="),
                          (dict(ws=None), b"null pointer"), (dict(bias=None), b"null pointer"), (dict(seeds=None), b"null pointer"),
                          (dict(pred=None), b"null pointer"), (dict(h=None), b"null pointer"),
                          (dict(ws_bytes=8 * 512 * 128 - 1), b"B needed"),
                          (dict(ws=native.c_ptr(4104)), b"16-byte aligned"), (dict(h=native.c_ptr(4100)), b"16-byte aligned")):
        assert call(**kwargs) != 0, kwargs
        err = lib.smt_last_error()
        assert NAME.encode() in err and words in err, (kwargs, err)
    # no rows: nothing is launched, the per-row pointers may be NULL
    assert call(rows=0, h=None, seeds=None, pred=None) == 0
    assert call(rows=0, cut=-1.5, h=None, seeds=None, pred=None) == 0


def test_op_refuses_bad_arguments_before_the_launch():
    from smt_amd import vqtts
    h, w, b, seeds = torch.zeros(8, 16), torch.zeros(32, 16), torch.zeros(32), torch.zeros(2, dtype=torch.int32)
    for t, mp in ((0.0, 0.0), (-1.0, 0.0), (INF, 0.0), (float("nan"), 0.0)):
        with pytest.raises(ValueError, match="temperature"):
            vqtts.code_head_sample(h, w, b, seeds, 4, t, mp)
    for mp in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="min_p"):
            vqtts.code_head_sample(h, w, b, seeds, 4, 1.0, mp)
    assert vqtts.sample_cut(2.0, 0.0) == (0.5, -INF) and vqtts.sample_cut(1.0, 1.0) == (1.0, 0.0)
    inv_t, cut = vqtts.sample_cut(0.7, 0.05)
    assert inv_t == 1 / 0.7 and cut == 0.7 * np.log(0.05) and S.device_scalars(0.7, 0.05) == (float(np.float32(inv_t)), float(np.float32(cut)))


def test_uniform_is_inside_the_unit_interval_and_exact_in_fp32():
    rng = np.random.default_rng(0)
    bits = np.concatenate([np.array([0, 2 ** 32 - 1, 511, 512, 2 ** 31], dtype=np.uint64), rng.integers(0, 2 ** 32, 100000, dtype=np.uint64)])
    u = S.uniform(bits)
    assert u.min() == 2.0 ** -24 and u.max() == 1 - 2.0 ** -24 and bool(((u > 0) & (u < 1)).all())
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)                       # representable
    # ... and the fp32 evaluation the device performs, (float)(bits >> 9) + 0.5f, then * 2^-23, rounds nowhere
    f = ((bits >> np.uint64(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)
    assert f.dtype == np.float32 and np.array_equal(f.astype(np.float64), u)
    g = -np.log(-np.log(u))
    assert bool(np.isfinite(g).all()) and g.min() > -2.9 and g.max() < 16.7


def test_keys_do_not_depend_on_the_batch_layout():
    assert int(S.fmix32(1)) == 0x514E28B7 and int(S.fmix32(0)) == 0                          # MurmurHash3's finaliser
    a = S.row_keys([5, 9, -1], 7).reshape(3, 7)
    b = S.row_keys([9, 5], 11).reshape(2, 11)
    assert np.array_equal(a[0], b[1, :7]) and np.array_equal(a[1], b[0, :7])
    assert len(set(a.reshape(-1).tolist())) == 21
    assert np.array_equal(S.row_keys([-1], 3), S.row_keys([2 ** 32 - 1], 3))                 # the (uint32) cast of an int32 seed


@pytest.mark.parametrize("temperature", [1.0, 0.7])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_helper_draws_from_the_tempered_softmax(temperature, seed):
    """65,536 draws at V = 32 against softmax(l / T), l ~ 1.5 N(0, 1): chi-square below the 99.9 % point at 31 degrees of
    freedom."""
    rows, bins = 65536, 32
    l = 1.5 * np.random.default_rng(100 + seed).standard_normal(bins)
    logits = np.broadcast_to(l, (rows, bins))
    d = S.draw64(logits, [seed, seed + 77, seed + 1234, -seed - 5], rows // 4, temperature)
    z = l * d["inv_t"]
    p = np.exp(z - z.max())
    p /= p.sum()
    chi = S.chi_square(np.bincount(d["pred"], minlength=bins), p)
    print(f"T={temperature} seed={seed}: chi-square {chi:.2f}")
    assert chi < S.CHI2_999[31]


def test_helper_truncates_to_the_kept_set():
    rows, bins = 65536, 32
    l = 1.5 * np.random.default_rng(7).standard_normal(bins)
    d = S.draw64(np.broadcast_to(l, (rows, bins)), [3, 4, 5, 6], rows // 4, 1.0, 0.2)
    kept = l >= l.max() + np.log(0.2)
    assert 2 <= kept.sum() < bins and np.array_equal(d["kept"][0], kept)
    counts = np.bincount(d["pred"], minlength=bins)
    assert not counts[~kept].any()
    p = np.where(kept, np.exp(l - l.max()), 0.0)
    assert S.chi_square(counts, p / p.sum()) < S.CHI2_999[int(kept.sum()) - 1]
    # min_p = 1 keeps the maxima alone
    d = S.draw64(np.broadcast_to(l, (8, bins)), [3], 8, 1.0, 1.0)
    assert bool((d["pred"] == l.argmax()).all()) and bool((d["kept"].sum(1) == 1).all())


def _model():
    from models.vqtts import VQTTS
    from utils import config as C
    return VQTTS(C.create(H.config_dict())).eval()


def test_infer_refuses_bad_sampling_arguments_without_a_device():
    model = _model()
    x, x_lens, _, _ = H.batch()
    for t in (-0.5, INF, float("nan")):
        with pytest.raises(ValueError, match="temperature"):
            model.infer(x, x_lens, temperature=t, seed=0)
    for mp in (-0.1, 1.01, float("nan")):
        with pytest.raises(ValueError, match="min_p"):
            model.infer(x, x_lens, temperature=1.0, min_p=mp, seed=0)
    with pytest.raises(ValueError, match="temperature = 0 is the argmax"):
        model.infer(x, x_lens, min_p=0.1)
    with pytest.raises(ValueError, match="temperature = 0 is the argmax"):
        model.infer(x, x_lens, seed=3)
    with pytest.raises(ValueError, match="needs seed"):
        model.infer(x, x_lens, temperature=1.0)
    for seeds in ([1, 2], [1, 2, 3, 4], torch.tensor([1, 2])):
        with pytest.raises(ValueError, match=f"sequence of {H.B} ints"):
            model.infer(x, x_lens, temperature=1.0, seed=seeds)
    with pytest.raises(ValueError, match=f"sequence of {H.B} ints"):
        model.infer(x, x_lens, temperature=1.0, seed=[1, 2.5, 3])
    # the predictor: a draw is a synthesis mode
    with pytest.raises(ValueError, match="target"):
        model.predictor(torch.zeros(1, 2, H.EMB), torch.zeros(1, 4, dtype=torch.int32), torch.tensor([4]),
                        target=torch.zeros(1, 4, dtype=torch.int64), sample=(1.0, 0.0, torch.zeros(1, dtype=torch.int32)))


def test_synthesize_refuses_bad_flags_without_a_device(tmp_path):
    from scripts import synthesize
    common = ["--log_dir", str(tmp_path), "--ckpt_num", "1", "--tokens", str(tmp_path / "none.txt")]
    args = synthesize.parse_args(common)
    assert args.temperature == 0.0 and args.min_p == 0.0 and args.seed == 0
    for flags, words in ((["--temperature", "-1"], "--temperature"), (["--temperature", "nan"], "--temperature"),
                         (["--temperature", "inf"], "--temperature"), (["--temperature", "1", "--min_p", "1.5"], "--min_p"),
                         (["--temperature", "1", "--min_p", "-0.5"], "--min_p"), (["--min_p", "0.1"], "--min_p")):
        with pytest.raises(ValueError, match=words):
            synthesize.main(common + flags)
