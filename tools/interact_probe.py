"""FM, CrossNetwork and CIN forward kernels and the FM / CrossNetwork backward (diagnostics), one process:

  fm      rf_fm_fwd, dense form, B 4096 x the cfg2 view [228 fields, 128 dims] f32 (no first order): reads B*228*128*4 bytes
  cross   rf_cross_fwd, B 4096 x 29184 f32, 3 layers: reads and writes B*29184*4 bytes each
  copy    rf_stream_copy of 1 GiB (read + write bytes / time; the best of its variants): the streaming HBM rate the two
          are stated against
  cin     rf_cin_fwd, B 4096, 200 fields x 128 dims bf16, cin_size [128, 128]: bf16 TFLOP/s from
          2 B D F0 H_k H_{k+1} FLOPs per layer
  torch   the reference's formulation composed from torch ops on the GPU in batch chunks: per layer the outer product
          [b, D, F0 * H_k] materialised in bf16, then a bf16 matmul with W_k (fp32 accumulate), X^{k+1} kept in fp32


Training legs (--legs train | all; written to --train-out, default profiles/interact/interact_train_probe.json), against
the same run's copy rate:
  fm_bwd     rf_fm_bwd, dense f32 [B, 228, 128]: must read x and write dx, 2 * B*228*128*4 bytes (its second read of the
             rows is meant to hit L2); torch = autograd's backward of the reference's formulation on the same GPU
  cross_bwd  rf_cross_bwd, [B, 29184] f32, 3 layers: must read x and dout and write dx, 3 * B*29184*4 bytes (the kernels
             read x and dout twice: 5 passes); torch = autograd's backward of the layer recursion
  steps      one step() of TrainableDeepFM and TrainableDCN: B 4096, 32 slots x D 64 (a [4096, 4096] embed output),
             250k bins per slot, hidden units (256, 128), DCN with 3 cross layers

CIN training leg (--legs cin_train only; written to --cin-train-out, default profiles/interact/cin_train_probe.json):
  cin_bwd    rf_cin_bwd at the forward leg's shape (B 4096, 200 fields x 128 dims bf16, cin_size [128, 128]; it runs the
             forward again), rf_cin_fwd beside it, and torch autograd (forward + backward) through the forward leg's
             bf16 composition in batch chunks, in the same process; --no-torch skips the composition
  step       one step() of TrainableXDeepFM at the step shape above (32 slots x D 64: CIN over [4096, 32, 128])

Timing: HIP events around `reps` back-to-back calls after `warm` warm-up calls; ms per call. Writes the JSON (default
profiles/interact/interact_probe.json).
    python tools/interact_probe.py [--out PATH] [--batch B] [--legs forward|train|all|cin_train]"""
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
ap.add_argument("--train-out", default=os.path.join(ROOT, "profiles", "interact", "interact_train_probe.json"))
ap.add_argument("--cin-train-out", default=os.path.join(ROOT, "profiles", "interact", "cin_train_probe.json"))
ap.add_argument("--legs", choices=["forward", "train", "all", "cin_train"], default="all")
ap.add_argument("--no-torch", action="store_true", help="cin_train: skip the torch autograd composition")
ap.add_argument("--step-reps", type=int, default=20)
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


def forward_legs():
    # --- FM -
    S, W2 = 228, 128
    enc = torch.randn((B, S * W2), device="cuda", generator=g)  # the encoder's [B, S * 2D] output
    ms = ev(lambda: N.fm_forward(embed=enc.view(B, S, W2)), args.reps, args.warm)
    nbytes = B * S * W2 * 4 + B * 4
    res["fm"] = {"shape": [B, S, W2], "ms": round(ms, 4), "bytes": nbytes, "GBs": round(nbytes / ms / 1e6, 1),
                 "frac_of_stream_copy": round(nbytes / ms / 1e6 / res["stream_copy_GBs"], 3)}

    # --- Cross -
    net = N.CrossNetwork(3, seed=1)
    ms = ev(lambda: net(enc), args.reps, args.warm)
    nbytes = 2 * B * S * W2 * 4 + 2 * 3 * S * W2 * 4
    res["cross"] = {"shape": [B, S * W2], "layers": 3, "ms": round(ms, 4), "bytes": nbytes, "GBs": round(nbytes / ms / 1e6, 1),
                    "frac_of_stream_copy": round(nbytes / ms / 1e6 / res["stream_copy_GBs"], 3)}
    del enc

    # --- CIN -
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


def train_legs():
    from recommendflow_amd.backend.encoder.sparse_encoder import FusedSparseEncoder, SlotSpec
    from recommendflow_amd.models.ranking.dcn import TrainableDCN
    from recommendflow_amd.models.ranking.deepfm import TrainableDeepFM
    from recommendflow_amd.runtime.batch import synthetic_batch

    out = {"batch": B, "device": res["device"], "stream_copy_GBs": res["stream_copy_GBs"]}
    copy = res["stream_copy_GBs"]
    S, W2 = 228, 128
    x = torch.randn((B, S * W2), device="cuda", generator=g)
    # --- rf_fm_bwd ---
    gout = torch.randn(B, device="cuda", generator=g)
    xv = x.view(B, S, W2)
    dx = torch.empty_like(xv)

    def fm_bwd():
        L.call("rf_fm_bwd", L.ptr(xv), L.DT_F32, xv.stride(0), xv.stride(1), None, None, 0, 0, B, S, W2, L.ptr(gout),
               L.ptr(dx), dx.stride(0), dx.stride(1), st)

    xr = xv.clone().requires_grad_(True)
    y = 0.5 * (torch.square(xr.sum(dim=1)) - torch.square(xr).sum(dim=1)).sum(dim=1)
    want = torch.autograd.grad(y, xr, gout, retain_graph=True)[0]
    fm_bwd()
    diff = float((dx - want).abs().max() / want.abs().max())
    ms = ev(fm_bwd, args.reps, args.warm)
    tms = ev(lambda: torch.autograd.grad(y, xr, gout, retain_graph=True), args.reps, args.warm)
    nbytes = 2 * B * S * W2 * 4 + B * 4
    out["fm_bwd"] = {"shape": [B, S, W2], "ms": round(ms, 4), "must_move_bytes": nbytes, "GBs": round(nbytes / ms / 1e6, 1),
                     "frac_of_stream_copy": round(nbytes / ms / 1e6 / copy, 3), "torch_autograd_ms": round(tms, 4),
                     "speedup_over_torch": round(tms / ms, 2), "max_rel_diff_vs_torch": diff}
    del xr, y, want, dx
    # --- rf_cross_bwd ---
    layers, dim = 3, S * W2
    net = N.TrainCrossNetwork(layers, seed=1)
    net.build((None, dim))
    w, b = net.w.detach(), net.b.detach()
    dout = torch.randn((B, dim), device="cuda", generator=g)
    dxc, dw, db = torch.empty_like(x), torch.empty_like(w), torch.empty_like(b)
    wsb = int(L.load().rf_cross_bwd_ws_bytes(B, dim, layers))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")

    def cross_bwd():
        L.call("rf_cross_bwd", L.ptr(x), L.DT_F32, dim, B, dim, layers, L.ptr(w), L.ptr(b), L.ptr(dout), dim, L.ptr(dxc), dim,
               L.ptr(dw), L.ptr(db), L.ptr(ws), wsb, st)

    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    xl = xr
    for l in range(layers):
        xl = xr * (xl * wr[l]).sum(dim=1, keepdim=True) + br[l] + xl
    wdx, wdw, wdb = torch.autograd.grad(xl, (xr, wr, br), dout, retain_graph=True)
    cross_bwd()

    def rel(pairs):
        return {k: float((a.double() - c).abs().max() / c.abs().max()) for k, (a, c) in pairs.items()}

    diff = rel({"dx": (dxc, wdx.double()), "dw": (dw, wdw.double()), "db": (db, wdb.double())})
    # both against the same recursion in float64 (torch autograd on the GPU)
    x6, w6, b6 = (t.double().requires_grad_(True) for t in (x, w, b))
    x6l = x6
    for l in range(layers):
        x6l = x6 * (x6l * w6[l]).sum(dim=1, keepdim=True) + b6[l] + x6l
    r6 = torch.autograd.grad(x6l, (x6, w6, b6), dout.double())
    err_fused = rel({"dx": (dxc, r6[0]), "dw": (dw, r6[1]), "db": (db, r6[2])})
    err_torch = rel({"dx": (wdx, r6[0]), "dw": (wdw, r6[1]), "db": (wdb, r6[2])})
    del x6, w6, b6, x6l, r6
    ms = ev(cross_bwd, args.reps, args.warm)
    tms = ev(lambda: torch.autograd.grad(xl, (xr, wr, br), dout, retain_graph=True), args.reps, args.warm)
    nbytes = 3 * B * dim * 4 + 4 * layers * dim * 4
    out["cross_bwd"] = {"shape": [B, dim], "layers": layers, "ms": round(ms, 4), "must_move_bytes": nbytes,
                        "moved_bytes": 5 * B * dim * 4, "ws_bytes": wsb, "GBs": round(nbytes / ms / 1e6, 1),
                        "frac_of_stream_copy": round(nbytes / ms / 1e6 / copy, 3),
                        "moved_frac_of_stream_copy": round(5 * B * dim * 4 / ms / 1e6 / copy, 3),
                        "torch_autograd_ms": round(tms, 4), "speedup_over_torch": round(tms / ms, 2),
                        "max_rel_diff_vs_torch": diff, "rel_err_vs_float64": err_fused,
                        "torch_f32_rel_err_vs_float64": err_torch}
    del xr, wr, br, xl, wdx, wdw, wdb, dxc, dout, x
    # --- one step() of each model ---
    SL, D, BINS = 32, 64, 250_000
    hb = synthetic_batch(B, [s % 2 == 1 for s in range(SL)], seed=3).to("cuda")
    yl = (torch.arange(B, device="cuda") % 2).float()
    steps = {}
    for name in ("deepfm", "dcn"):
        specs = [SlotSpec(f"f{s}", BINS, (2022, 2023), ["sum", "avg"][s % 2]) for s in range(SL)]
        enc = FusedSparseEncoder(specs, D, seed=4)
        model = TrainableDeepFM(enc, seed=1) if name == "deepfm" else TrainableDCN(enc, layer_num=3, seed=1)
        ms = ev(lambda: model.step(hb, yl), args.step_reps, 5)
        steps[name] = {"B": B, "slots": SL, "D": D, "embed_width": SL * 2 * D, "table_rows": enc.table_rows,
                       "hidden_units": [256, 128], "step_ms": round(ms, 3)}
        del model, enc
    out["steps"] = steps
    os.makedirs(os.path.dirname(os.path.abspath(args.train_out)), exist_ok=True)
    with open(args.train_out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


def cin_train_leg():
    import ctypes

    from recommendflow_amd.backend.encoder.sparse_encoder import FusedSparseEncoder, SlotSpec
    from recommendflow_amd.models.ranking import TrainableXDeepFM
    from recommendflow_amd.runtime.batch import synthetic_batch

    out = {"batch": B, "device": res["device"], "stream_copy_GBs": res["stream_copy_GBs"]}
    F0, D, sizes = 200, 128, [128, 128]
    K, sumH = len(sizes), sum(sizes)
    x = (torch.rand((B, F0, D), device="cuda", generator=g) * 2 - 1).to(torch.bfloat16)
    cin = N.TrainCIN(sizes, seed=2)
    cin.build(x.shape)
    Hk = F0
    for i, H in enumerate(sizes):
        cin.cin_W[f"CIN_W_{i}"].data.copy_(torch.randn((1, F0 * Hk, H), device="cuda", generator=g) / (F0 * Hk) ** 0.5)
        Hk = H
    cin.refresh()
    packed, packed_t = cin._packed, cin._pack_transposed()
    dout = torch.randn((B, sumH), device="cuda", generator=g)
    lib = L.load()
    wsb = int(lib.rf_cin_bwd_ws_bytes(B, F0, D, cin._sizes, K))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    dx = torch.empty((B, F0, D), dtype=torch.float32, device="cuda")
    dWs = [torch.empty_like(cin.cin_W[f"CIN_W_{i}"].data) for i in range(K)]
    ptrs = (ctypes.c_void_p * K)(*[d.data_ptr() for d in dWs])

    def bwd():
        L.call("rf_cin_bwd", L.ptr(x), L.DT_BF16, x.stride(0), x.stride(1), B, F0, D, cin._sizes, K, L.ptr(packed),
               L.ptr(packed_t), L.ptr(dout), dout.stride(0), L.ptr(dx), dx.stride(0), dx.stride(1), ptrs, L.ptr(ws), wsb, st)

    with torch.no_grad():
        fwd_ms = ev(lambda: cin(x), args.cin_reps, 1)
    bwd_ms = ev(bwd, args.cin_reps, 1)
    flops, Hk = 0, F0
    for H in sizes:
        flops += 2 * B * D * F0 * Hk * H
        Hk = H
    leg = {"shape": [B, F0, D], "cin_size": sizes, "x_dtype": "bf16", "forward_flops": flops, "backward_flops": 3 * flops,
           "ws_bytes": wsb, "packed_w_bytes": packed.numel(), "packed_w_t_bytes": packed_t.numel(),
           "rf_cin_fwd_ms": round(fwd_ms, 3), "rf_cin_bwd_ms": round(bwd_ms, 3),
           "rf_cin_bwd_TFLOPs": round(3 * flops / bwd_ms / 1e9, 1),
           "bwd_over_fwd": round(bwd_ms / fwd_ms, 2), "bwd_over_3x_design_fwd_33.4ms": round(bwd_ms / (3 * 33.4), 2)}
    if not args.no_torch:
        Wl = [cin.cin_W[f"CIN_W_{i}"].data[0].to(torch.bfloat16).requires_grad_(True) for i in range(K)]

        def composed(xc):
            b = xc.shape[0]
            x0 = xc.permute(0, 2, 1)
            xk, outs = x0.float(), []
            for W in Wl:
                outer = (x0.unsqueeze(3) * xk.to(torch.bfloat16).unsqueeze(2)).reshape(b * D, -1)
                xk = torch.matmul(outer, W).float().view(b, D, -1)
                outs.append(xk.sum(dim=1))
            return torch.cat(outs, dim=1)

        def torch_train():
            """forward + backward per batch chunk: dx per chunk, the dW of the chunks accumulated by autograd"""
            for W in Wl:
                W.grad = None
            dxs = []
            for i in range(0, B, args.chunk):
                xc = x[i: i + args.chunk].detach().requires_grad_(True)
                (composed(xc) * dout[i: i + args.chunk]).sum().backward()
                dxs.append(xc.grad)
            return torch.cat(dxs, dim=0)

        def torch_fwd():
            with torch.no_grad():
                return [composed(x[i: i + args.chunk]) for i in range(0, B, args.chunk)]

        tf_ms = ev(torch_fwd, 1, 1)
        tt_ms = ev(torch_train, 1, 1)
        want = torch_train()
        bwd()
        leg.update({"torch_chunk": args.chunk, "torch_forward_ms": round(tf_ms, 3),
                    "torch_forward_backward_ms": round(tt_ms, 3), "torch_backward_ms": round(tt_ms - tf_ms, 3),
                    "speedup_fwd_plus_bwd_over_torch": round(tt_ms / (fwd_ms + bwd_ms), 2),
                    "speedup_bwd_over_torch_backward": round((tt_ms - tf_ms) / bwd_ms, 2),
                    "dx_rel_diff_vs_torch": float((dx - want.float()).abs().max() / want.float().abs().max()),
                    "dW_rel_diff_vs_torch": [float((dWs[i][0] - Wl[i].grad.float()).abs().max() /
                                                   Wl[i].grad.float().abs().max()) for i in range(K)]})
        del Wl, want
    out["cin_bwd"] = leg
    del x, dx, ws, dout, dWs
    SL, DD, BINS = 32, 64, 250_000
    hb = synthetic_batch(B, [s % 2 == 1 for s in range(SL)], seed=3).to("cuda")
    yl = (torch.arange(B, device="cuda") % 2).float()
    specs = [SlotSpec(f"f{s}", BINS, (2022, 2023), ["sum", "avg"][s % 2]) for s in range(SL)]
    enc = FusedSparseEncoder(specs, DD, seed=4)
    model = TrainableXDeepFM(enc, seed=1)
    ms = ev(lambda: model.step(hb, yl), args.step_reps, 5)
    out["step"] = {"B": B, "slots": SL, "D": DD, "embed_width": SL * 2 * DD, "table_rows": enc.table_rows,
                   "hidden_units": [256, 128], "cin_size": [128, 128], "step_ms": round(ms, 3)}
    os.makedirs(os.path.dirname(os.path.abspath(args.cin_train_out)), exist_ok=True)
    with open(args.cin_train_out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if args.legs == "cin_train":
    cin_train_leg()
if args.legs in ("forward", "all"):
    forward_legs()
if args.legs in ("train", "all"):
    train_legs()
