"""TransformerEncoder training: rf_tfenc_fwd and rf_tfenc_bwd against torch autograd through the bf16 composition, one
process (diagnostics), at the four shapes of tools/tfenc_probe.py:

  fwd        transformer_encoder_stack(blocks, x, mask): the one-launch forward
  bwd        rf_tfenc_bwd through the ABI (images packed beforehand), and its kernels one by one from torch.profiler
             (null if the profiler gives no device events)
  torch      torch autograd through the composition in bf16 (matmul, softmax, layer_norm; the [B, heads, L, L]
             probabilities and every arrow in HBM), forward and forward + backward, chunked over the batch
  step       one TrainableTabTransformer.step() on a synthetic batch with L slots of width d (first shape only)

FLOPs per example and block of what rf_tfenc_bwd runs: the chain again 6 L d^2 + 4 L^2 d + 4 L d ffn (the stack's forward
for the blocks below the last one comes on top), the weight and input gradients 12 L d^2 + 8 L d ffn, and the two
attention sweeps 2 x 8 L^2 d (S and dP are computed in both): 18 L d^2 + 20 L^2 d + 12 L d ffn, against the 3 x forward
(18 L d^2 + 12 L^2 d + 12 L d ffn) of a backward that stores what it needs.
    python tools/tfenc_train_probe.py [--out PATH] [--batch B] [--reps N]"""
import argparse
import ctypes
import json
import math
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from recommendflow_amd.backend.layers import network_layers as N  # noqa: E402
from recommendflow_amd.runtime import lib as L  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tfenc", "tfenc_train_probe.json"))
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warm", type=int, default=1)
ap.add_argument("--chunk", type=int, default=512)
args = ap.parse_args()
L.load()
L.require_gpu()
B = args.batch


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


def torch_block(x, P, mask, heads):
    F = torch.nn.functional
    Bn, Ln, d = x.shape
    sp = lambda t: t.view(Bn, Ln, heads, d // heads).transpose(1, 2)  # noqa: E731
    q, k, v = (x @ P[n + "_kernel"].t() + P[n + "_bias"] for n in ("wq", "wk", "wv"))
    logits = sp(q) @ sp(k).transpose(-1, -2) / math.sqrt(d // heads)
    logits = logits.masked_fill(mask.view(Bn, 1, Ln, 1) == 0, -4294967295.0)
    att = (F.softmax(logits.float(), dim=-1).to(x.dtype) @ sp(v)).transpose(1, 2).reshape(Bn, Ln, d)
    out1 = F.layer_norm(x + att, (d,), P["ln1_gamma"], P["ln1_beta"], 1e-6)
    ffn = F.relu(out1 @ P["conv1_kernel"].t() + P["conv1_bias"]) @ P["conv2_kernel"].t() + P["conv2_bias"]
    return F.layer_norm(out1 + ffn, (d,), P["ln2_gamma"], P["ln2_beta"], 1e-6)


g = torch.Generator(device="cuda").manual_seed(7)
res = {"batch": B, "device": torch.cuda.get_device_name(0)}
legs = []
for Ln, d, heads, ffn in ((228, 128, 2, 128), (39, 128, 4, 256)):
    x = torch.randn((B, Ln, d), device="cuda", generator=g)
    mask = (torch.rand((B, Ln), device="cuda", generator=g) >= 0.3).float()
    dout = torch.randn((B, Ln, d), device="cuda", generator=g)
    for nb in (1, 3):
        blocks = [N.TrainTransformerEncoder(d, num_heads=heads, ffn_hidden_unit=ffn, seed=10 * i) for i in range(nb)]
        for blk in blocks:
            blk.eval()
        out = torch.empty((B, Ln, d), dtype=torch.float32, device="cuda")
        fwd_ms = ev(lambda: N.transformer_encoder_stack(blocks, x, mask, out=out), args.reps, args.warm)
        packed = blocks[0]._stack[1]
        packed_t = N._tfenc_pack_transposed(blocks)
        wsb = int(L.load().rf_tfenc_bwd_ws_bytes(B, Ln, d, heads, ffn, nb))
        ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
        dx = torch.empty_like(x)
        shapes = {"wq_kernel": (d, d), "wk_kernel": (d, d), "wv_kernel": (d, d), "conv1_kernel": (d, ffn),
                  "conv2_kernel": (ffn, d), "conv1_bias": (ffn,)}
        grads = [torch.empty(shapes.get(nm, (d,)), device="cuda") for _ in range(nb) for nm in N._TFENC_ABI]
        ptrs = (ctypes.c_void_p * len(grads))(*[t.data_ptr() for t in grads])

        def bwd():
            L.call("rf_tfenc_bwd", L.ptr(x), L.DT_F32, x.stride(0), x.stride(1), L.ptr(mask), B, Ln, d, heads, ffn, nb,
                   L.ptr(packed), L.ptr(packed_t), 1e-6, L.ptr(dout), dout.stride(0), dout.stride(1), L.ptr(dx), dx.stride(0),
                   dx.stride(1), ptrs, L.ptr(ws), ws.numel(), L.stream_ptr())

        bwd_ms = ev(bwd, args.reps, args.warm)
        kernels = None
        try:
            from torch.profiler import ProfilerActivity, profile

            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                bwd()
                torch.cuda.synchronize()
            kernels = {}
            for e in prof.key_averages():
                t = getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0)
                if t:
                    hit = re.search(r"(tfb_\w+|tfenc_\w+)", e.key)
                    name = hit.group(1) if hit else e.key[:60]
                    kernels[name] = round(kernels.get(name, 0.0) + t / 1e3, 3)
            kernels = kernels or None
        except Exception as exc:  # diagnostics only
            kernels = {"error": repr(exc)[:200]}

        Ps = [{nm: getattr(blk, nm).detach().to(torch.bfloat16).requires_grad_(True) for nm in N._TFENC_ABI} for blk in blocks]
        ch = min(args.chunk, B)

        def torch_run(backward):
            for c0 in range(0, B, ch):
                xc = x[c0: c0 + ch].to(torch.bfloat16).requires_grad_(backward)
                with torch.set_grad_enabled(backward):
                    y = xc
                    for P in Ps:
                        y = torch_block(y, P, mask[c0: c0 + ch], heads)
                if backward:
                    y.backward(dout[c0: c0 + ch].to(torch.bfloat16))

        tf_ms = ev(lambda: torch_run(False), max(1, args.reps // 2), 1)
        tfb_ms = ev(lambda: torch_run(True), max(1, args.reps // 2), 1)
        fwd_flops = nb * B * (6 * Ln * d * d + 4 * Ln * Ln * d + 4 * Ln * d * ffn)
        bwd_flops = nb * B * (18 * Ln * d * d + 20 * Ln * Ln * d + 12 * Ln * d * ffn) + (nb - 1) * fwd_flops // nb
        legs.append({"shape": [B, Ln, d], "heads": heads, "ffn": ffn, "blocks": nb, "ws_bytes": wsb,
                     "fwd_ms": round(fwd_ms, 3), "bwd_ms": round(bwd_ms, 3), "bwd_kernels_ms": kernels,
                     "fwd_flops": fwd_flops, "bwd_flops": bwd_flops,
                     "bwd_ms_flop_proportional_to_fwd": round(fwd_ms * bwd_flops / fwd_flops, 3),
                     "torch_bf16_fwd_ms": round(tf_ms, 3), "torch_bf16_fwd_bwd_ms": round(tfb_ms, 3), "torch_chunk": ch,
                     "fused_fwd_bwd_vs_torch": round(tfb_ms / (fwd_ms + bwd_ms), 2)})
        print(json.dumps(legs[-1]), flush=True)
        del blocks, out, ws, grads, Ps
    del x, mask, dout
res["legs"] = legs

try:
    from recommendflow_amd.backend.encoder.sparse_encoder import FusedSparseEncoder, SlotSpec
    from recommendflow_amd.models.ranking import TrainableTabTransformer
    from recommendflow_amd.runtime.batch import synthetic_batch

    S, D = 228, 64
    enc = FusedSparseEncoder([SlotSpec(f"f{s}", 1000, (2022, 2023), "sum") for s in range(S)], D, seed=4)
    model = TrainableTabTransformer(enc, n_blocks=1, num_heads=2, ffn_hidden_unit=128, hidden_units=(256, 128), dropout=0.3)
    hb = synthetic_batch(B, [False] * S, seed=3, id_max=900, uniform=True).to("cuda")
    y = (torch.arange(B, device="cuda") % 2).float()
    res["tabtransformer_step"] = {"slots": S, "dim": D, "blocks": 1, "heads": 2, "ffn": 128,
                                  "step_ms": round(ev(lambda: model.step(hb, y), 3, 1), 3)}
except Exception as exc:  # diagnostics only
    res["tabtransformer_step"] = {"error": repr(exc)[:300]}

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
