# What a fill of the two-column kernel spends outside its chain: the launch stamps of sw_systolic2.inc (s2_stamp: debug_buf slots
# 8 n + 32 + k behind the strips' own, 100 MHz ticks) for the planner's scan, the shared scan (debug bit 28) and the private one (bit 29).
# usage: python scripts/prologue_stamps.py [cols rows] ...      (default: 16384 16384); run on the GPU box
import importlib, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sw = importlib.import_module("smith-waterman_amd")
nums = [int(x) for x in sys.argv[1:]]
shapes = list(zip(nums[0::2], nums[1::2])) or [(16384, 16384)]
eng = sw.Engine(0)
print("cols rows scan | us from workgroup 0's entry to: last workgroup's entry, alphabet known by all, prologue left by all, strip 0's first step | "
      "last stores acknowledged -> last workgroup out | entry -> out", flush=True)
for cols, rows in shapes:
    a, b = sw.generate(cols, rows, 1)
    d_a, _ = eng.to_device(a)
    d_b, _ = eng.to_device(b)
    out = eng.alloc(cols, rows)
    for name, flags in (("planner", 0), ("barrier", 1 << 28), ("scan_all", 1 << 29)):
        eng.set_option("debug_flags", flags)
        for _ in range(3):
            eng.fill_into(out, d_a, d_b)
        eng.synchronize()
        rec = []
        for _ in range(5):
            dbg = torch.zeros(16 * ((cols + 62) // 63) + 256, dtype=torch.int64, device=out.res.device)
            eng.set_option("debug_buf", dbg.data_ptr())
            eng.fill_into(out, d_a, d_b)
            eng.synchronize()
            eng.set_option("debug_buf", 0)
            n = int(eng.get_option("last_strips2"))
            if n <= 0 or eng.get_option("last_tiles") != 1:
                break
            t = dbg.cpu().numpy()[8 * n + 32: 8 * n + 39].astype(np.float64) / 100.0   # us
            rec.append([t[6] - t[0], t[1] - t[0], t[2] - t[0], t[3] - t[0], t[5] - t[4], t[5] - t[0]])
        eng.set_option("debug_flags", 0)
        if not rec:
            print(cols, rows, name, "(not one launch of the two-column kernel)", flush=True)
            continue
        m = np.median(np.array(rec), axis=0)
        print(f"{cols} {rows} {name} scan_all={eng.get_option('last_scan_all')} | {m[0]:.2f} {m[1]:.2f} {m[2]:.2f} {m[3]:.2f} | {m[4]:.2f} | {m[5]:.1f}", flush=True)
eng.close()
