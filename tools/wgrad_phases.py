"""Per-phase cycle sums of conv_wgrad_shift_kernel from the -DSMT_WGRAD_STAMP=1 build (tools/wgrad_phases.sh): cycles per
128-row tile and wave spent in: wait + barrier at the top of the tile | staging issue before the k-loop | k-loop (with
whatever staging is issued inside it) | and, once per workgroup, the slab store.  The stamp after the k-loop does not wait
for the last MFMAs, so their drain shows up in the next tile's barrier column: read the sum."""
import ctypes, os, sys
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "speech-masters-thesis_amd"))
from smt_amd import convops as C, native

B, T, dt = 32, int(os.environ.get("T", 72704)), torch.bfloat16
g = torch.Generator(device="cuda").manual_seed(0)
x = torch.randn(B, T, 128, device="cuda", generator=g).to(dt)
dy = torch.randn(B, T, 128, device="cuda", generator=g).to(dt)
lib = ctypes.CDLL(native.LIB_PATH)
names = ["barrier", "stage", "k-loop"]
for k, dil in [(3, 1), (5, 3), (7, 9), (9, 27)]:
    pad = (k - 1) * dil // 2
    dw, db = torch.empty(128, 128, k, device="cuda"), torch.empty(128, device="cuda")

    def run():
        d = C._base_desc(x, dy, None, 128, 128, k, 1, dil, pad, T)
        C._wgrad(d, dw, 128 * k, k, 1, list(range(k)), db)

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
    per = a[:, :, :3] / np.maximum(tiles[:, :, None], 1)
    m = per[live].mean(axis=0)
    print(f"k={k} dil={dil}: {s.elapsed_time(e) * 1e3:.1f} us (wgrad + reduce), tiles per workgroup {tiles[live].mean():.1f}; "
          f"cycles per tile (mean over waves)")
    print("   " + "  ".join(f"{n} {v:7.0f}" for n, v in zip(names, m)) + f"   sum {m.sum():7.0f}"
          f"   mfma bound {512 * k:5d}   slab store (per workgroup) {a[:, :, 3][live].mean():7.0f}")
