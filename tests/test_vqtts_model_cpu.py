"""The assembled VQTTS without a GPU: the emission entry point is declared, bound and exported under the unchanged ABI number,
the model constructs from its configuration with the reference's parameter tree (tests/golden/vqtts_model_keys.json, written
from the reference's own class), the synthetic token + audio dataset keeps its contract, and train.py accepts the names."""
import json
import os
import re

import pytest
import torch

import vqtts_model_helpers as H
from conftest import GOLDEN, PKG, REPO

CSRC = os.path.join(PKG, "csrc")


def _config(**model_overrides):
    from utils import config as C
    cfg = C.create(H.config_dict())
    cfg.model.update(C.create(model_overrides))
    return cfg


def test_emit_entry_point_is_declared_bound_and_exported():
    from smt_amd import native
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "smt_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(smt_\w+)\s*\(", header))
    assert "smt_vqtts_emit" in declared and "smt_vqtts_emit" in native.exported_symbols()
    assert declared == set(native.exported_symbols())
    abi = int(re.search(r"smt_abi_version\(void\)\s*\{\s*return\s+(\d+)", open(os.path.join(CSRC, "common.hip")).read()).group(1))
    lib = native.lib()
    assert abi == native.ABI_VERSION == lib.smt_abi_version()
    assert hasattr(lib, "smt_vqtts_emit")
    res, args = native._SIGNATURES["smt_vqtts_emit"]
    assert res is native.c_int and len(args) == 14 and args[5:11] == [native.c_int] * 6
    # argument errors are decided on the host, before any launch: they need no GPU
    assert lib.smt_vqtts_emit(None, None, None, None, None, 1, 1, 1, 1, 1, 6, None, None, None) != 0
    assert b"multiple of 4" in lib.smt_last_error()
    assert lib.smt_vqtts_emit(None, None, None, None, None, 0, 5, 7, 3, 2, 8, None, None, None) == 0      # batch 0: no-op
    assert lib.smt_vqtts_emit(None, None, None, None, None, 2, 5, 0, 3, 2, 8, None, None, None) == 0      # t_q 0
    assert lib.smt_vqtts_emit(None, None, None, None, None, 2, 5, 7, 3, 2, 0, None, None, None) == 0      # dim 0
    assert lib.smt_vqtts_emit(None, None, None, None, None, 2, 5, 7, 3, 2, 8, None, None, None) != 0      # null pointers


def test_emit_codes_refuses_bad_arguments_before_the_launch():
    from smt_amd import vqtts
    with pytest.raises(ValueError, match="device tensor"):
        vqtts.emit_codes(torch.zeros(1, 1, dtype=torch.int32), torch.zeros(1, 1, dtype=torch.int64), torch.zeros(1, 1, dtype=torch.int32),
                         torch.zeros(1, dtype=torch.int32), torch.zeros(4, 8), 2, 2)


def test_constructs_from_the_yaml_configuration():
    from models.vqtts import VQTTS
    from utils import config as C
    from utils.commons import get_model
    cfg = C.merge(C.load(os.path.join(PKG, "configs/models/vqtts.yaml")), C.load(os.path.join(PKG, "configs/datasets/synthetic_vqtts.yaml")),
                  C.create({"train": {"batch_size": 2, "n_gpus": 1, "ema": False}}))
    model, _ = get_model(cfg, "cpu")
    assert isinstance(model, VQTTS) and cfg.dataset.use_spect is False and cfg.dataset.use_audio and cfg.dataset.use_token
    assert model.stride == 256 and 145408 // model.stride == 568                  # the frame of the reference geometry
    assert model.quant_bottleneck.k.shape == (149 * 512, 128)                       # (148 ids + blank) groups of 512 codes
    assert model.audio_encoder.level_blocks[0].blocks[0].weight.shape[0] == 64      # width * multipliers[-1]
    assert len(model.audio_encoder.level_blocks) == 3 and len(model.audio_decoder.level_blocks) == 3
    # the reference's own configuration carries the same values for every key it has
    ref_keys = dict(levels=3, downs_t=[3, 3, 2], strides_t=[2, 2, 2], l_bins=512, emb_width=128, multipliers=[2, 1, 1], width=64, depth=3)
    assert all(cfg.model[k] == v for k, v in ref_keys.items())
    assert cfg.model.loss.align == 0.1 and cfg.model.loss.log is False and cfg.optimizer.eps == 1e-9


def test_parameter_tree_is_the_references():
    from models.vqtts import VQTTS
    with open(os.path.join(GOLDEN, "vqtts_model_keys.json")) as f:
        ref = {k: tuple(v) for k, v in json.load(f).items()}
    model = VQTTS(_config())
    mine = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    # the two stated exceptions: the grouped codebook has n_vocab * l_bins rows where the reference builds the flat block's
    # l_bins, and the DFT bases of the spectral loss are derived data here
    groups = H.N_VOCAB + 1
    assert ref["quant_bottleneck.k"] == (H.L_BINS, H.EMB) and mine["quant_bottleneck.k"] == (groups * H.L_BINS, H.EMB)
    basis = {k for k in ref if k.endswith("_basis")}
    assert len(basis) == 6 and not any(k.endswith("_basis") for k in mine)
    want = {k: v for k, v in ref.items() if k not in basis}
    want["quant_bottleneck.k"] = mine["quant_bottleneck.k"]
    assert mine == want
    tops = {k.split(".")[0] for k in mine}
    assert tops == {"text_encoder", "audio_encoder", "audio_decoder", "quant_bottleneck", "quant_decoder", "quant_proj"}
    for i in range(4):
        assert mine[f"quant_decoder.model.{i}.model.2.weight"] == (2 * H.EMB, H.EMB, 3)
        assert mine[f"quant_decoder.model.{i}.model.5.weight"] == (H.EMB, 2 * H.EMB, 1)
    assert mine["quant_proj.weight"] == (H.L_BINS, H.EMB, 1)


def test_state_dict_round_trips_and_parameters_appear_once():
    from models.vqtts import VQTTS
    torch.manual_seed(0)
    a, b = VQTTS(_config()), VQTTS(_config())
    sd = {k: torch.randn_like(v) for k, v in a.state_dict().items()}
    sd["multi_stft_loss.stfts.0.forward_basis"] = torch.zeros(3)               # a reference checkpoint's extra: dropped on load
    missing, unexpected = b.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    back = b.state_dict()
    assert set(back) == set(sd) - {"multi_stft_loss.stfts.0.forward_basis"}
    assert all(torch.equal(back[k], sd[k]) for k in back)
    with pytest.raises(RuntimeError):
        b.load_state_dict({k: v for k, v in sd.items() if k != "quant_proj.weight"}, strict=True)
    names = [n for n, _ in b.named_parameters()]
    assert len(names) == len(set(names)) and len({id(p) for _, p in b.named_parameters()}) == len(names)
    assert len(list(b.parameters())) == len(names)
    floats = {k for k, v in back.items() if v.is_floating_point() and k != "quant_bottleneck.k"}       # k is a buffer
    assert set(names) == floats
    # the predictor computes with the very parameters the model registers, and follows train() / eval()
    assert b.predictor.quant_proj.weight is dict(b.named_parameters())["quant_proj.weight"]
    assert b.predictor.quant_decoder is b.quant_decoder
    assert b.eval().predictor.training is False and b.train().predictor.training is True
    assert b.double().predictor.quant_proj.weight.dtype == torch.float64       # what .to() / _apply reaches


def test_dropout_sites_of_the_stacks_are_disjoint():
    from models.vqtts import VQTTS
    from models.vqtts.vqtts import PREDICTOR_SEED_BIT
    from smt_amd.convops import dropout_key
    m = VQTTS(_config())
    ids = m.dropout_sites()
    n_audio = m.audio_encoder.n_sites + m.audio_decoder.n_sites
    assert n_audio == 2 * (3 + 3 + 2) * 2 * 2                                  # 8 blocks per stack, 2 sites per branch, depth 2
    assert sorted(ids.values()) == list(range(len(ids))) and len(ids) > n_audio
    assert all((i < n_audio) == n.startswith("audio_") for n, i in ids.items())
    # one step's keys: the audio stacks and the text encoder under (seed, site), the predictor's eight under its own seed
    for seed in (1, 2, 12345):
        keys = [dropout_key(seed, s) for s in ids.values()] + [dropout_key(seed | PREDICTOR_SEED_BIT, s) for s in range(8)]
        assert len(set(keys)) == len(keys)


def test_speakers_are_refused():
    from models.vqtts import VQTTS
    with pytest.raises(ValueError, match="n_speakers"):
        VQTTS(_config(n_speakers=2))


def test_synthetic_tts_audio_dataset():
    from datasets.ljspeech import TRUNC_MOD
    from datasets.synthetic import SyntheticTTSAudio
    from utils import config as C
    assert TRUNC_MOD == 512
    for ragged in (False, True):
        cfg = C.load(os.path.join(PKG, "configs/datasets/synthetic_vqtts.yaml"))
        cfg.dataset.update(C.create(dict(num_clips=6, clip_length=16384, max_tokens=24, ragged=ragged)))
        train, val = SyntheticTTSAudio(cfg, "train"), SyntheticTTSAudio(cfg, "val")
        assert len(train) == 6 and len(val) == 10
        items = [train[i] for i in range(6)]
        for token, tx, spect, spect_len, audio, t, speaker in items:
            assert spect is None and spect_len is None and speaker is None
            assert token.dtype == torch.int64 and token.shape == (tx,) and 1 <= tx <= 24
            assert int(token.min()) >= 0 and int(token.max()) < 149                      # 148 ids + the blank
            assert audio.dtype == torch.float32 and audio.shape == (t,) and t % 512 == 0 and t > 0
            assert t // 256 >= tx                                                       # a frame for every token
            assert float(audio.abs().max()) <= 1.0 and float(audio.std()) > 0.05
        again = SyntheticTTSAudio(cfg, "train")[3]
        assert torch.equal(again[0], items[3][0]) and torch.equal(again[4], items[3][4])          # seeded
        assert not torch.equal(val[3][4][:4096], items[3][4][:4096])                              # the splits differ
        if not ragged:
            assert all(it[5] == 16384 for it in items)
        batch = SyntheticTTSAudio.collate(items[:4])
        assert batch[0].dtype == torch.int64 and batch[0].shape == (4, max(it[1] for it in items[:4]))
        assert batch[1].tolist() == [it[1] for it in items[:4]] and batch[2] is None and batch[3] is None and batch[6] is None
        assert batch[4].shape == (4, 1, max(it[5] for it in items[:4])) and batch[5].tolist() == [it[5] for it in items[:4]]
    # the audio depends on the token under it: one-token clips of different ids differ in their tone
    cfg = C.load(os.path.join(PKG, "configs/datasets/synthetic_vqtts.yaml"))
    cfg.dataset.update(C.create(dict(clip_length=8192, max_tokens=2, n_vocab=3, intersperse_blanks=False)))
    seen = {}
    for i in range(40):
        token, tx, _, _, audio, _, _ = SyntheticTTSAudio(cfg, "train")[i]
        if tx != 1:
            continue
        spec = torch.fft.rfft(audio[:2048].double() * torch.hann_window(2048, dtype=torch.float64)).abs()
        seen.setdefault(int(token[0]), set()).add(int(spec[2:40].argmax()) + 2)
    assert set(seen) == {1, 2} and seen[1].isdisjoint(seen[2])                          # f0 170 Hz vs 250 Hz: bins ~16 vs ~23


def test_train_py_accepts_the_names(monkeypatch):
    import train
    from models.vqtts import VQTTS
    from utils.commons import _resolve
    monkeypatch.chdir(PKG)
    args = train.parse_args(["--model", "vqtts", "--dataset", "synthetic_vqtts", "--batch_size", "4"])
    cfg = train.build_config(args)
    assert _resolve(cfg.model["_import_"]) is VQTTS
    assert cfg.dataset["_import_"] == "datasets.synthetic.SyntheticTTSAudio" and cfg.train.batch_size == 4
    assert _resolve(cfg.dataset["_import_"]).__name__ == "SyntheticTTSAudio"
