"""FM, CrossNetwork and CIN forward kernels (diagnostics), one process:

  fm      rf_fm_fwd, dense form, B 4096 x the cfg2 view [228 fields, 128 dims] f32 (no first order): reads B*228*128*4 bytes
  cross   rf_cross_fwd, B 4096 x 29184 f32, 3 layers: reads and writes B*29184*4 bytes each
  copy    rf_stream_copy of 1 GiB (read + write bytes / time; the best of its variants): the streaming HBM rate the two
          are stated against
  cin     rf_cin_fwd, B 4096, 200 fields x 128 dims bf16, cin_size [128, 128]: bf16 TFLOP/s from
          2 B D F0 H_k H_{k+1} FLOPs per layer
  torch   the reference's formulation composed from torch ops on the GPU in batch chunks: per layer the outer product
          [b, D, F0 * H_k] materialised in bf16, then a bf16 matmul with W_k (fp32 accumulate), X^{k+1} kept in fp32

Timing: HIP events around `reps` back-to-back calls after `warm` warm-up calls; ms per call. Writes the JSON (default
profiles/interact/interact_probe.json).
    python tools/interact_probe.py [--out PATH] [--batch B]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from recommendflow_amd.backend.layers import network_layers as N  # noqa: E402
from recommendflow_amd.runtime import lib as L  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "interact", "interact_probe.json"))
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warm", type=int, default=3)
ap.add_argument("--cin-reps", type=int, default=3)
ap.add_argument("--chunk", type=int, default=128, help="examples per chunk of the torch composition")
args = ap.parse_args()
L.load()
L.require_gpu()
B = args.batch
st = L.stream_ptr()


def ev(fn, reps, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


g = torch.Generator(device="cuda").manual_seed(7)
res = {"batch": B, "device": torch.cuda.get_device_name(0)}

# --- the streaming rate -----------------------------------------------------------------------------------------------
n = 1 << 30
src = torch.empty(n, dtype=torch.uint8, device="cuda").zero_()
dst = torch.empty_like(src)
copy_ms = min(ev(lambda v=v: L.call("rf_stream_copy", L.ptr(src), L.ptr(dst), n, v, st), 10, 2) for v in range(4))
res["stream_copy_GBs"] = round(2 * n / copy_ms / 1e6, 1)
del src, dst

# --- FM ---------------------------------------------------------------------------------------------------------------
S, W2 = 228, 128
enc = torch.randn((B, S * W2), device="cuda", generator=g)  # the encoder's [B, S * 2D] output
ms = ev(lambda: N.fm_forward(embed=enc.view(B, S, W2)), args.reps, args.warm)
nbytes = B * S * W2 * 4 + B * 4
res["fm"] = {"shape": [B, S, W2], "ms": round(ms, 4), "bytes": nbytes, "GBs": round(nbytes / ms / 1e6, 1),
             "frac_of_stream_copy": round(nbytes / ms / 1e6 / res["stream_copy_GBs"], 3)}

# --- Cross ------------------------------------------------------------------------------------------------------------
net = N.CrossNetwork(3, seed=1)
ms = ev(lambda: net(enc), args.reps, args.warm)
nbytes = 2 * B * S * W2 * 4 + 2 * 3 * S * W2 * 4
res["cross"] = {"shape": [B, S * W2], "layers": 3, "ms": round(ms, 4), "bytes": nbytes, "GBs": round(nbytes / ms / 1e6, 1),
                "frac_of_stream_copy": round(nbytes / ms / 1e6 / res["stream_copy_GBs"], 3)}
del enc

# --- CIN --------------------------------------------------------------------------------------------------------------
F0, D, sizes = 200, 128, [128, 128]
x = (torch.rand((B, F0, D), device="cuda", generator=g) * 2 - 1).to(torch.bfloat16)
cin = N.CIN(sizes, seed=2)
cin.build(x.shape)
Hk = F0
for i, H in enumerate(sizes):
    cin.cin_W[f"CIN_W_{i}"].data.copy_(torch.randn((1, F0 * Hk, H), device="cuda", generator=g) / (F0 * Hk) ** 0.5)
    Hk = H
cin.refresh()
Ws = [cin.cin_W[f"CIN_W_{i}"].data[0].to(torch.bfloat16) for i in range(len(sizes))]


def composed(xc):
    """One batch chunk of the reference's steps: outer product [b, D, F0 * H_k] in bf16, then the 1x1 conv as a matmul."""
    b = xc.shape[0]
    x0 = xc.permute(0, 2, 1)  # [b, D, F0]
    xk, outs = x0.float(), []
    for W in Ws:
        outer = (x0.unsqueeze(3) * xk.to(torch.bfloat16).unsqueeze(2)).reshape(b * D, -1)  # materialised, bf16
        xk = torch.matmul(outer, W).float().view(b, D, -1)
        outs.append(xk.sum(dim=1))
    return torch.cat(outs, dim=1)


def composed_all():
    return torch.cat([composed(x[i: i + args.chunk]) for i in range(0, B, args.chunk)], dim=0)


fused_ms = ev(lambda: cin(x), args.cin_reps, 1)
torch_ms = ev(composed_all, 1, 1)
got, want = cin(x), composed_all()
flops, Hk = 0, F0
for H in sizes:
    flops += 2 * B * D * F0 * Hk * H
    Hk = H
res["cin"] = {"shape": [B, F0, D], "cin_size": sizes, "x_dtype": "bf16", "flops": flops, "fused_ms": round(fused_ms, 3),
              "fused_TFLOPs": round(flops / fused_ms / 1e9, 1), "torch_composition_ms": round(torch_ms, 3),
              "torch_chunk": args.chunk, "speedup": round(torch_ms / fused_ms, 2),
              "fused_vs_torch_rel_diff": float((got - want).abs().max() / want.abs().max())}

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
