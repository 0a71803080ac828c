"""Per-phase cycle sums of conv_wgrad_kernel (the generic weight-gradient kernel) from a -DSMT_WGRAD_STAMP=1 build of
conv_wgrad.hip (tools/wgrad_phases.sh builds one): cycles per staged tile and wave spent in: the two barriers of a tile |
global loads -> LDS stores done | the k-loop (with the next tile's load issue, where the build prefetches) | and, once per
workgroup, the slab store.  Shapes: the three bf16 instances of the flagship step (k = 4 stride-2 down conv, the two 2-tap
phases of its transpose, a 3-tap conv), batch 32, at the largest (72,704 rows) and smallest (1,136 rows) resampling level.
The stamps cover workgroups 0..255 only; the time is wgrad + reduce of one call."""
import ctypes, os, sys
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "speech-masters-thesis_amd"))
from smt_amd import convops as C, native

B, bf = 32, torch.bfloat16
lib = ctypes.CDLL(native.LIB_PATH)
names = ["barrier", "stage", "k-loop"]
g = torch.Generator(device="cuda").manual_seed(0)
for t in (72704, 1136):
    for kind in ("down", "up0", "up1", "k3"):
        if kind == "down":
            t_in, t_y, taps, stride, pad, os_, oo = 2 * t, t, 4, 2, 1, 1, 0
        elif kind == "k3":
            t_in, t_y, taps, stride, pad, os_, oo = t, t, 3, 1, 1, 1, 0
        else:
            t_in, t_y, taps, stride, os_ = t, 2 * t, 2, 1, 2
            pad, oo = (1, 0) if kind == "up0" else (0, 1)
        x = torch.randn(B, t_in, 64, device="cuda", generator=g).to(bf)
        dy = torch.randn(B, t_y, 64, device="cuda", generator=g).to(bf)
        dw, db = torch.empty(64, 64, taps, device="cuda"), torch.empty(64, device="cuda")

        def run():
            d = C._base_desc(x, dy, None, 64, 64, taps, stride, 1, pad, t, t_y=t_y, out_stride=os_, out_offset=oo)
            C._wgrad(d, dw, 64 * taps, taps, 1, list(range(taps)), db)

        for _ in range(3):
            run()
        torch.cuda.synchronize()
        buf = (ctypes.c_ulonglong * (256 * 64))()
        lib.smt_wgrad_debug_dump(buf, 256 * 64, 1)
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        run()
        e.record(); torch.cuda.synchronize()
        lib.smt_wgrad_debug_dump(buf, 256 * 64, 1)
        a = np.array(buf, dtype=np.float64).reshape(256, 8, 8)
        tiles = a[:, :, 4]
        live = tiles > 0
        m = (a[:, :, :3] / np.maximum(tiles[:, :, None], 1))[live].mean(axis=0)
        nbytes = B * (t_in * 128 + t * 128)
        print(f"{kind:5s} t_out {t:6d}: {s.elapsed_time(e) * 1e3:7.1f} us (wgrad + reduce, {nbytes / 1e6:6.1f} MB of operands), "
              f"tiles per workgroup {tiles[live].mean():5.1f}; cycles per tile (mean over waves)")
        print("      " + "  ".join(f"{n} {v:7.0f}" for n, v in zip(names, m)) + f"   sum {m.sum():7.0f}"
              f"   mfma bound {512 * (taps + 1):4d}   slab store (per workgroup) {a[:, :, 3][live].mean():7.0f}", flush=True)
