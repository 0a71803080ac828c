"""Shared by the VQTTS model tests and tests/golden/make_golden_vqtts_model.py: the test configuration, and a float64 CPU
restatement of the model's training forward composed from the oracles.  Nothing here imports the product at import time
(the fixture script imports this file with the reference first on the path).

The test configuration is the smallest at which every stage still has its edges: the reference geometry (levels 3, downs_t
[3, 3, 2], strides_t [2, 2, 2]: one frame = 256 samples) at width 32, depth 2, multipliers [1, 1, 1]; code width 64; a
text encoder of 2 layers, 2 heads, window 4, prenet, mean_only; vocabulary 11 + the blank = 12 groups; the reference's loss
block with linf_topk 256.  Two sizes are not the ones first planned for this configuration, because kernels that are not
this model's to change refuse those with an argument error, and the smallest size they accept stands in:
  * l_bins is 32, not 16: the grouped quantiser (smt_vq_grouped_forward) and the code head (smt_vqtts_code_head_fwd) take
    a multiple of 32 bins (tests/test_vqtts_align_gpu.py::test_module_feeds_bottleneck_gather_and_length_loss stands in the
    same way);
  * the text encoder is hidden 64, filter 128, not hidden 32, filter 64: its fused residual + LayerNorm
    (smt_lm_add_ln_fwd) takes a channel count that is a multiple of 64 ("dim must be a multiple of 64 up to 2048 (got
    32)"); 64 / 128 is the text encoder of tests/test_glow_gpu.py."""
import math

N_VOCAB, L_BINS, EMB = 11, 32, 64
B, T, TX = 3, 8192, 12
Y_LENS, X_LENS, Q_LENS = (8192, 6144, 4096), (12, 7, 5), (32, 24, 16)
STRIDE = 256


def config_dict(dropout=0.0, p_dropout=0.0):
    """{"model": ..., "dataset": ...} as plain dicts: the keys both the reference's VQTTS and this build's read."""
    enc = dict(n_vocab=N_VOCAB, out_channels=EMB, hidden_channels=64, filter_channels=128, filter_channels_dp=128, kernel_size=3,
               p_dropout=p_dropout, n_layers=2, n_heads=2, window_size=4, prenet=True, mean_only=True)
    loss = dict(commit=0.05, multispectral=1.0, align=0.1, l1=0.0, l2=1.0, linf=0.02, linf_topk=256, n_ffts=[2048, 1024, 512],
                hop_lengths=[240, 120, 50], win_lengths=[1200, 600, 240], window="hann", log=False)
    model = dict(_import_="models.vqtts.vqtts.VQTTS", n_speakers=1, gin_channels=0, encoder=enc, levels=3, downs_t=[3, 3, 2],
                 strides_t=[2, 2, 2], emb_width=EMB, l_bins=L_BINS, mu=0.99, multipliers=[1, 1, 1], width=32, depth=2, m_conv=1.0,
                 revival_threshold=1.0, use_bottleneck=True, dilation_growth_rate=3, dilation_cycle=None, kernel_size_growth_rate=2,
                 kernel_size_cycle=None, reverse_decoder_dilation=True, zero_out=True, block_type="gated_hifi", ddi=False, loss=loss,
                 compute_dtype="fp32", dropout=dropout)
    dataset = dict(intersperse_blanks=True, cmudict_path="", sample_rate=22050, n_fft=1024, hop_length=256, win_length=1024, n_mels=80)
    return {"model": model, "dataset": dataset}


def batch(seed=0):
    """(x [B, Tx] int64, x_lens, y [B, 1, T] fp32, y_lens): ragged token ids in [0, 12) and audio whose segments depend on
    the token under them (a tone per id plus noise), so that the alignment has something to find."""
    import torch
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, N_VOCAB + 1, (B, TX), generator=g)
    y = torch.zeros(B, 1, T)
    t = torch.arange(T, dtype=torch.float64) / 22050.0
    for b in range(B):
        n, tx = Y_LENS[b], X_LENS[b]
        owner = (torch.arange(T) * tx // n).clamp(max=tx - 1)
        f0 = 200.0 + 150.0 * x[b, owner].double()
        y[b, 0] = (0.4 * torch.sin(2 * math.pi * f0 * t) + 0.2 * (torch.rand(T, generator=g, dtype=torch.float64) * 2 - 1)).float()
    return x, torch.tensor(X_LENS), y, torch.tensor(Y_LENS)


def randomize_zero_init(model, seed=1):
    """Every zero-initialised tensor (the `.model.5` convs of the residual layers, the prenet's projection, ...) gets seeded
    values, so that no gradient is vacuously zero.  Weights +-1 / sqrt(fan_in), biases +-0.1."""
    import torch
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if bool((p == 0).all()):
                bound = 0.1 if p.dim() == 1 else 1.0 / math.sqrt(p[0].numel())
                p.copy_(((torch.rand(p.shape, generator=g) * 2 - 1) * bound).to(p.device))


def predictor_stack64(p, x, valid):
    """The code predictor's residual stack in float64 (models/vqtts/predictor.py: dilations 27, 9, 3, 1; rows at or past
    q_lens read as zero by every conv), on x [B, Tq, C] with the 0/1 row mask valid [B, Tq, 1]."""
    import torch
    import torch.nn.functional as F
    for i, dil in enumerate([27, 9, 3, 1]):
        x = x * valid
        u = F.conv1d(torch.relu(x).transpose(1, 2), p[f"quant_decoder.model.{i}.model.2.weight"],
                     p[f"quant_decoder.model.{i}.model.2.bias"], padding=dil, dilation=dil)
        u = torch.relu(u) * valid.transpose(1, 2)
        x = x + F.conv1d(u, p[f"quant_decoder.model.{i}.model.5.weight"], p[f"quant_decoder.model.{i}.model.5.bias"]).transpose(1, 2)
    return x * valid


def forward64(p, k0, x, x_lens, y, y_lens, align_idx, q_rel, cfg):
    """The training forward of models/vqtts/vqtts.py restated on the CPU in the dtype of ``p`` (float64 in the tests).  The
    discrete results are teacher-forced -- ``align_idx`` [B, Tq] (-1 = no token) and ``q_rel`` [B, Tq] come from the device
    run -- and everything continuous is recomputed from the parameters ``p`` (state-dict names) and the pre-step codebook
    ``k0``.  Composed from oracle.glow_oracle.text_encoder, oracle.vqvae_oracle.encoder_forward / decoder_forward and its
    two loss functions.  No dropout.  Returns the loss dict of VQTTS.forward plus q_acc."""
    import torch
    from oracle import glow_oracle as go
    from oracle import vqvae_oracle as orc
    m = cfg["model"]
    ocfg = orc.VQVAEConfig.from_dict(m)
    l_bins, l_align = m["l_bins"], m["loss"]["align"]
    y = y.to(k0.dtype)
    p_text = {"encoder." + k[len("text_encoder."):]: v for k, v in p.items() if k.startswith("text_encoder.")}
    x_m, _, logw, x_mask = go.text_encoder(x, x_lens, p_text, {"encoder": m["encoder"]}, go.no_dropout)
    y_mask = orc.sequence_mask(y_lens, y.shape[2]).unsqueeze(1).to(y.dtype)
    y_enc, q_mask = orc.encoder_forward(y, y_mask, p, ocfg, prefix="audio_encoder")
    x_e, y_e = x_m.transpose(1, 2), y_enc.transpose(1, 2)                       # [B, Tx, D], [B, Tq, D]
    q_lens = q_mask[:, 0].sum(-1).long()
    d = y_e.shape[-1]
    idx = align_idx.long()
    has = idx >= 0
    gather = idx.clamp(min=0)
    x_g = torch.gather(x_e, 1, gather[..., None].expand(-1, -1, d))              # matmul(x_enc, attn) of the reference
    # alignment loss on the path, duration loss against the path's durations
    loss_align = (x_g - y_e)[has].pow(2).sum(-1).sqrt().sum() / (x_lens * q_lens).sum()
    dur = torch.zeros(x.shape, dtype=y.dtype).scatter_add_(1, gather, has.to(y.dtype))
    loss_dur = (((logw - torch.log(1e-8 + dur)) ** 2) * x_mask[:, 0]).sum() / x_lens.sum()
    # grouped quantiser: straight-through rows, commit over the frames with a token
    tok = torch.gather(x, 1, gather)
    y_q = k0[tok * l_bins + q_rel.long()]
    hm = has.to(y.dtype)[..., None]
    loss_commit = (((y_q - y_e) ** 2) * hm).sum() / (has.sum() * d)
    y_d = (y_e + (y_q - y_e).detach()) * hm
    # code predictor on the detached text side
    valid = (torch.arange(idx.shape[1])[None, :] < q_lens[:, None])
    h = predictor_stack64(p, (x_g * hm).detach(), valid.to(y.dtype)[..., None])
    logits = h @ p["quant_proj.weight"][:, :, 0].t() + p["quant_proj.bias"]
    scored = valid & has
    loss_ce = torch.nn.functional.cross_entropy(logits[scored], q_rel.long()[scored])
    q_acc = (logits[scored].argmax(-1) == q_rel.long()[scored]).to(y.dtype).mean()
    # audio decoder and the waveform losses
    y_h, _ = orc.decoder_forward(y_d.transpose(1, 2), q_mask, p, ocfg, prefix="audio_decoder")
    loss_recon = orc.multinorm_recon_loss(y, y_h, y_mask, ocfg)
    loss_stft = orc.multires_stft_loss(y, y_h, y_mask, ocfg)
    loss = (loss_recon + m["loss"]["multispectral"] * loss_stft + m["loss"]["commit"] * loss_commit + loss_dur + l_align * loss_align
            + loss_ce)
    return {"loss": loss, "loss_recon": loss_recon, "loss_stft": loss_stft, "loss_commit": loss_commit, "loss_dur": loss_dur,
            "loss_align": loss_align / (1 + l_align), "loss_ce": loss_ce, "yh": y_h.squeeze(1), "q_acc": q_acc}
