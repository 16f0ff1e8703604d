#!/usr/bin/env python3
"""In-kernel timeline of the fused dense-block kernel (build with -DNESR_RDB_ABL=256): per step, cycles (s_memtime) that
MFMA wave 1 and DMA wave 0 of workgroup 77 spend waiting at the barrier / computing / issuing DMAs / in the epilogue.
usage: tools/probes/rdb_stamps.py build/v_stamps.so"""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
from tools.ab import load, make_ctx
from neural_enhanced_super_resolution_amd.synth import synthetic_state_dict
lib = load(os.path.abspath(sys.argv[1]))
sd = synthetic_state_dict(seed=0, num_in_ch=3, scale=2)
ctx = make_ctx(lib, sd, 3)
x = torch.rand(1, 3, 512, 512, device="cuda")
y = torch.empty(1, 3, 1024, 1024, device="cuda")
st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
for _ in range(5):
    assert lib.nesr_forward(ctx, ctypes.c_void_p(x.data_ptr()), 1, 3, 512, 512, ctypes.c_void_p(y.data_ptr()), st) == 0
torch.cuda.synchronize()
buf = (ctypes.c_ulonglong * (2 * 64 * 8))()
lib.nesr_debug_rdb_stamps.argtypes = [ctypes.c_void_p]
assert lib.nesr_debug_rdb_stamps(buf) == 0
S = [[[buf[(r * 64 + s) * 8 + e] for e in range(8)] for s in range(64)] for r in range(2)]
# steps of a dense block: the kernel says (older builds: 52, conv5 as two passes of 32 output channels)
N = lib.nesr_debug_rdb_steps() if hasattr(lib, "nesr_debug_rdb_steps") else 52
t0 = min(S[0][0][0], S[1][0][0])
print("step | MFMA: arrive  wait  compute | DMA: arrive(vm wait) barrier-wait  issue  epilogue | step length")
for s in range(N):
    m, d = S[0][s], S[1][s]
    nm = S[0][s + 1][0] if s < N - 1 else m[2]
    nd = S[1][s + 1][0] if s < N - 1 else d[3]
    ep = ""
    if m[3] > m[1] and m[6] > m[3]:
        ep = f"  epilogue in the MFMA wave: start +{m[3]-m[1]} exchange/bias/act {m[4]-m[3]} split/regroup {m[5]-m[4]} stores {m[6]-m[5]}"
    print(f"{s:3d} | {m[0]-t0:8d} {m[1]-m[0]:6d} {m[2]-m[1]:6d} | {d[0]-t0:8d} ({d[1]-d[0]:5d}) {d[2]-d[1]:6d} {d[3]-d[2]:6d} {nd-d[3]:6d} | {nm-m[0]:6d}{ep}")
print("total cycles", S[0][N - 1][2] - t0)
# outside the steps (slot 61): [role][61][0] = kernel entry of that wave, [0][61][1] = the final epilogue's last store has
# retired (the stamp build waits for it).  The DMA wave's step-0 stamp is its first instruction behind the first barrier.
if S[1][61][0] and S[0][61][1]:
    print(f"entry -> first barrier: DMA wave 0 {S[1][0][0] - S[1][61][0]} cycles (MFMA wave 1 entered {S[0][61][0] - S[1][61][0]:+d} relative to it)")
    print(f"last step -> end: {S[0][61][1] - S[0][N - 1][2]} cycles (MFMA wave 1: end of the last MFMA step to its last store retired)")
    print(f"entry -> end: {S[0][61][1] - min(S[0][61][0], S[1][61][0])} cycles")
# a chained launch (rdb_f16x2_chain_kernel): the table holds the launch's last block; slot 59 = the block in front of it:
# [0][59][0] end of its last MFMA step, [0][59][1] its last store retired, [1][59][0..1] DMA wave 0 at / behind the block's last
# barrier, [1][59][2] the nine tiles' level 5 seen in the last block's re-entry
if S[0][59][0]:
    e = S[0][59][0]
    print("block boundary of the chained launch (last block but one -> last block), cycles after the end of the last MFMA step:")
    print(f"  last store retired {S[0][59][1] - e}, last barrier released {S[1][59][1] - e}, the nine tiles' level 5 seen {S[1][59][2] - e}, "
          f"first barrier released (DMA wave 0's step-0 stamp) {S[1][0][0] - e}, MFMA wave 1 behind barrier 0 {S[0][0][1] - e}")
    print(f"  last MFMA step -> first MFMAs of the next block: {S[0][0][1] - e} cycles")
dr, dt = S[1][63][0] - S[1][62][0], S[1][63][1] - S[1][62][1]
print(f"steps 0..{N - 1}: {dt} shader cycles in {dr} ticks of the 100 MHz clock = {dr / 100:.2f} us: shader clock {dt / dr * 100:.0f} MHz")

arr = (ctypes.c_ulonglong * (12 * 8 * 2))()
lib.nesr_debug_rdb_arrive.argtypes = [ctypes.c_void_p]
if lib.nesr_debug_rdb_arrive(arr) == 0:
    print("barrier arrival of every wave (MFMA 0-7, DMA 8-11) relative to the release of that barrier, steps 20..27")
    for st in range(8):
        rel = max(arr[(w * 8 + st) * 2 + 0] for w in range(12))
        print(20 + st, " ".join(f"{int(arr[(w * 8 + st) * 2 + 0]) - int(rel):6d}" for w in range(12)),
              "| release seen", " ".join(f"{int(arr[(w * 8 + st) * 2 + 1]) - int(rel):5d}" for w in range(12)))

tp = (ctypes.c_ulonglong * (2 * 8 * 8))()
if hasattr(lib, "nesr_debug_rdb_taps"):
    lib.nesr_debug_rdb_taps.argtypes = [ctypes.c_void_p]
    if lib.nesr_debug_rdb_taps(tp) == 0:
        print("tap-steps of MFMA waves 1 and 5 (the two of one SIMD), steps 20..27: start of tap-step 0..4 and end, relative to wave 1's tap-step 0")
        for st in range(8):
            b = int(tp[(0 * 8 + st) * 8 + 0])
            for w in range(2):
                print(20 + st, "wave", 1 + 4 * w, " ".join(f"{int(tp[(w * 8 + st) * 8 + i]) - b:6d}" for i in range(6)))
