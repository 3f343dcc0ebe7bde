"""Compile-time ablations of the d=512 single-head attention kernel on the GPU box (sdm_bench_attn, qt bit 64).  Bench helper.
usage: python tools/attn_d512_ablate.py [--pp | --pp-noprio]      (the ping-pong form attn_d512_pp_kernel, qt bit 256; without s_setprio: bit 32)"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package
load_package()
from comfyui_sdmatte_amd.engine import Engine
from comfyui_sdmatte_amd.config import SDMatteConfig
eng = Engine(SDMatteConfig.tiny(), 0, precision="fp16x3")
QT = 64 | (256 if "--pp" in sys.argv or "--pp-noprio" in sys.argv else 0) | (32 if "--pp-noprio" in sys.argv else 0)
print({64: "attn_d512_kernel", 320: "attn_d512_pp_kernel", 352: "attn_d512_pp_kernel without s_setprio"}[QT])
names = {0: "full", 1: "no exchange / softmax", 6: "no MFMAs", 7: "no MFMAs, no softmax (DMAs + fragment reads + barriers)", 8: "no DMAs", 32: "no fragment reads",
         40: "no DMAs, no fragment reads", 41: "MFMAs + barriers only"}
for (B, Lq, Lk) in [(8, 16384, 16384), (4, 16384, 16384)]:
    fl = 4.0 * B * Lq * Lk * 512
    print(f"B={B} Lq={Lq} Lk={Lk} d=512")
    for ab in (0, 0, 1, 6, 7, 8, 32, 40, 41):
        ms = eng.bench_attn(B, 1, Lq, Lk, qt=QT, ablate=ab, iters=3)
        print(f"   ablate={ab:2d} {names[ab]:60s} {ms:8.4f} ms  ({fl / ms / 1e9:8.1f} TF/s equiv)")
eng.close()
