"""Que2Search AttentionFusion backward and training step (diagnostics), one process:

  per shape (B 4096, C 6, d 64) and (B 4096, C 16, d 256), is_norm = 1:
    fused      rf_attention_fusion_bwd (dx + deterministic dW), and with dW = NULL (the dx / dl pass alone)
    composite  the same backward as autograd of torch ops on the GPU (softmax(x @ W), weighted sum, l2 normalise)
    copy       rf_stream_copy of B*C*d*4 bytes: 2*B*C*d*4 bytes of traffic, the x read and the dx write of the backward
  one TrainableQue2Search.step() at a cfg-like shape (B 4096, 2 user + 6 ad slots, D 64, dim 128, 250k-bin slots).

Timing: HIP events around `reps` back-to-back calls after `warm` warm-up calls; ms per call. The small shape's
kernels take microseconds, so its figures are bounded by the launch rate of the three (fused) or dozen (composite)
launches, not by memory. Writes the JSON (default profiles/que2search/que2search_probe.json).
    python tools/que2search_probe.py [--out PATH] [--reps R]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from recommendflow_amd.runtime import lib as L  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "que2search", "que2search_probe.json"))
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--warm", type=int, default=10)
ap.add_argument("--step-reps", type=int, default=30)
args = ap.parse_args()
L.load()
L.require_gpu()


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


def composite(x, W, C, d):
    att = torch.softmax(x @ W, dim=1)
    u = (x.view(x.shape[0], C, d) * att.unsqueeze(-1)).sum(dim=1)
    ss = (u * u).sum(dim=1, keepdim=True)
    return u * torch.rsqrt(torch.clamp(ss, min=1e-12))


def shape_row(B, C, d):
    g = torch.Generator(device="cuda").manual_seed(7)
    K = C * d
    x = torch.randn((B, K), device="cuda", generator=g)
    W = (torch.rand((K, C), device="cuda", generator=g) * 2 - 1) * (6.0 / (K + C)) ** 0.5
    dout = torch.randn((B, d), device="cuda", generator=g)
    out = torch.empty((B, d), device="cuda")
    att = torch.empty((B, C), device="cuda")
    st = L.stream_ptr()
    L.call("rf_attention_fusion_fwd", L.ptr(x), B, C, d, K, L.ptr(W), 1, L.ptr(out), d, L.ptr(att), st)
    dx, dW = torch.empty_like(x), torch.empty_like(W)
    wsb = int(L.load().rf_attention_fusion_bwd_ws_bytes(B, C, d))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")

    def fused(dw):
        L.call("rf_attention_fusion_bwd", L.ptr(x), B, C, d, K, L.ptr(W), 1, L.ptr(att), L.ptr(dout), d, L.ptr(dx), K,
               L.ptr(dw), L.ptr(ws), wsb, st)

    xr, Wr = x.clone().requires_grad_(True), W.clone().requires_grad_(True)
    y = composite(xr, Wr, C, d)
    cdx, cdW = torch.autograd.grad(y, (xr, Wr), dout, retain_graph=True)
    fused(dW)
    torch.cuda.synchronize()
    agree = {"dx": float((dx - cdx).abs().max() / cdx.abs().max()), "dW": float((dW - cdW).abs().max() / cdW.abs().max())}
    dst = torch.empty_like(x)
    nbytes = B * K * 4
    t_fused = ev(lambda: fused(dW), args.reps, args.warm)
    t_dx = ev(lambda: fused(None), args.reps, args.warm)
    t_comp = ev(lambda: torch.autograd.grad(y, (xr, Wr), dout, retain_graph=True), args.reps, args.warm)
    t_copy = ev(lambda: L.call("rf_stream_copy", L.ptr(x), L.ptr(dst), nbytes, 0, st), args.reps, args.warm)
    return {"B": B, "C": C, "d": d, "is_norm": 1, "traffic_bytes": 2 * nbytes, "ws_bytes": wsb,
            "fused_ms": round(t_fused, 4), "fused_dx_only_ms": round(t_dx, 4), "composite_ms": round(t_comp, 4),
            "stream_copy_ms": round(t_copy, 4), "fused_over_composite": round(t_comp / t_fused, 2),
            "fused_vs_copy_rate": round(t_copy / t_fused, 3), "dx_only_vs_copy_rate": round(t_copy / t_dx, 3),
            "fused_GBps_of_traffic": round(2 * nbytes / t_fused / 1e6, 1),
            "copy_GBps": round(2 * nbytes / t_copy / 1e6, 1), "max_rel_diff_vs_composite": agree}


def step_row():
    from recommendflow_amd.backend.encoder.sparse_encoder import FusedSparseEncoder, SlotSpec
    from recommendflow_amd.models.matching.que2search import TrainableQue2Search
    from recommendflow_amd.runtime.batch import synthetic_batch

    B, S, NU, D, DIM, BINS = 4096, 8, 2, 64, 128, 250_000
    specs = [SlotSpec(f"f{s}", BINS, (2022, 2023), ["sum", "avg"][s % 2]) for s in range(S)]
    enc = FusedSparseEncoder(specs, D, seed=4)
    model = TrainableQue2Search(enc, NU, DIM, seed=1)
    hb = synthetic_batch(B, [s % 2 == 1 for s in range(S)], seed=3).to("cuda")
    y = (torch.arange(B, device="cuda") % 2).float()
    ms = ev(lambda: model.step(hb, y), args.step_reps, 5)
    return {"B": B, "user_slots": NU, "ad_slots": S - NU, "D": D, "dim": DIM, "table_rows": enc.table_rows,
            "loss": "cosent", "step_ms": round(ms, 3)}


res = {"device": torch.cuda.get_device_name(0), "reps": args.reps,
       "backward": [shape_row(4096, 6, 64), shape_row(4096, 16, 256)], "step": step_row()}
print(json.dumps(res))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
