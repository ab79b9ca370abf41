"""TransformerEncoder: the fused launch (rf_tfenc_fwd through transformer_encoder_stack) against the composition of the
operators the library already had, one process (diagnostics):

  fused     transformer_encoder_stack(blocks, x, mask): one launch for all blocks, x f32 [B, L, d] read in place
  composed  per block: MultiHeadAttention.call (three Dense in exact fp32, the casts to bf16, rf_sdpa_fwd), a torch add,
            rf_norm_fwd via Norm (f32 out), the two Dense of FFN (exact fp32), another add and Norm; every arrow is a
            [B L, d] fp32 tensor in HBM
  copy      rf_stream_copy of 1 GiB (read + write bytes / time; the best of its variants), in the same run

Shapes: (L 228, d 128, heads 2, ffn 128), the workload's [4096, 228, 128] view, and (L 39, d 128, heads 4, ffn 256),
with 1 and 3 blocks, B 4096. FLOPs per example and block: 6 L d^2 (projections) + 4 L^2 d (QK^T, PV) + 4 L d ffn.
Timing: HIP events around `reps` back-to-back calls after `warm` warm-up calls; ms per call. Writes the JSON (default
profiles/tfenc/tfenc_probe.json).
    python tools/tfenc_probe.py [--out PATH] [--batch B] [--reps N]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tfenc", "tfenc_probe.json"))
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warm", type=int, default=2)
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

n = 1 << 30
src = torch.empty(n, dtype=torch.uint8, device="cuda").zero_()
dst = torch.empty_like(src)
copy_ms = min(ev(lambda v=v: L.call("rf_stream_copy", L.ptr(src), L.ptr(dst), n, v, st), 10, 2) for v in range(4))
res["stream_copy_GBs"] = round(2 * n / copy_ms / 1e6, 1)
del src, dst


def composed_block(blk, x, mask):
    Bn, Ln, d = x.shape
    att = blk.mha.call(x, x, x, mask)
    out1 = blk.layernorm1((x + att).reshape(Bn * Ln, d), out_dtype=torch.float32)
    ffn = blk.ffn.conv2(blk.ffn.conv1(out1))
    return blk.layernorm2(out1 + ffn, out_dtype=torch.float32).reshape(Bn, Ln, d)


legs = []
for Ln, d, heads, ffn in ((228, 128, 2, 128), (39, 128, 4, 256)):
    x = torch.randn((B, Ln, d), device="cuda", generator=g)
    mask = (torch.rand((B, Ln), device="cuda", generator=g) >= 0.3).float()
    for nb in (1, 3):
        blocks = [N.TransformerEncoder(d, num_heads=heads, ffn_hidden_unit=ffn, seed=10 * i) for i in range(nb)]
        for blk in blocks:
            blk.mha.dtype = torch.bfloat16  # the attention core of the composition on bf16 operands, as the fused kernel
        out = torch.empty((B, Ln, d), dtype=torch.float32, device="cuda")

        def fused():
            return N.transformer_encoder_stack(blocks, x, mask, out=out)

        def composed():
            y = x
            for blk in blocks:
                y = composed_block(blk, y, mask)
            return y

        fused_ms = ev(fused, args.reps, args.warm)
        comp_ms = ev(composed, args.reps, args.warm)
        got, want = fused().clone(), composed()
        flops = nb * B * (6 * Ln * d * d + 4 * Ln * Ln * d + 4 * Ln * d * ffn)
        # per block the kernel reads its input, writes x + att, reads it back and writes its output (L2 hits included)
        io_bytes = nb * 4 * B * Ln * d * 4
        legs.append({"shape": [B, Ln, d], "heads": heads, "ffn": ffn, "blocks": nb, "flops": flops,
                     "fused_ms": round(fused_ms, 3), "fused_TFLOPs": round(flops / fused_ms / 1e9, 1),
                     "fused_global_bytes": io_bytes,
                     "fused_global_bytes_ms_at_stream_copy": round(io_bytes / res["stream_copy_GBs"] / 1e6, 3),
                     "composed_ms": round(comp_ms, 3), "composed_TFLOPs": round(flops / comp_ms / 1e9, 1),
                     "speedup": round(comp_ms / fused_ms, 2),
                     "fused_vs_composed_rel_diff": float((got - want).abs().max() / want.abs().max())})
        del blocks, out, got, want
    del x, mask
res["legs"] = legs
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
