"""cfg5 recall search with an IVF index (diagnostics): FaissSearcher "IVF1024,Flat" against "Flat" in the same
process, 1024 l2-normalised queries x 1M items x 256, top-200, nprobe in {1, 4, 16, 64, 1024}.

Data: a mixture of 16384 Gaussian clusters on the unit sphere (item = centre + noise, normalised; query = an item +
noise, normalised; about 61 items a cluster, so a top-200 spans several clusters and lists), so that the lists have
something to find; i.i.d. directions have no neighbourhoods to index.
Timing: no graph; per configuration two warm-up searches, then HIP events around `reps` searches, each on a query
batch of its own (the batches are drawn ahead). Reports ms per search, recall@200 against Flat on the first batch,
the train time and Flat's ms, and writes the JSON (default profiles/ivf/ivf_search_probe.json).
    python tools/ivf_probe.py [--out PATH] [--reps R] [--items N]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from recommendflow_amd.backend.third_party_components.faiss_searcher import FaissSearcher  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivf", "ivf_search_probe.json"))
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--items", type=int, default=1_000_000)
ap.add_argument("--nprobe", type=int, nargs="*", default=[1, 4, 16, 64, 1024])
args = ap.parse_args()

N, E, B, K, NLIST, WARM, NCLUSTER = args.items, 256, 1024, 200, 1024, 2, 16384
g = torch.Generator(device="cuda").manual_seed(3)


def unit(x):
    return x / x.norm(dim=1, keepdim=True)


centres = unit(torch.randn((NCLUSTER, E), device="cuda", generator=g))
items = unit(centres[torch.randint(0, NCLUSTER, (N,), device="cuda", generator=g)]
             + 0.5 / E ** 0.5 * torch.randn((N, E), device="cuda", generator=g))
batches = [unit(items[torch.randint(0, N, (B,), device="cuda", generator=g)]
                + 0.3 / E ** 0.5 * torch.randn((B, E), device="cuda", generator=g)) for _ in range(WARM + args.reps)]

ivf = FaissSearcher(items=items.cpu().numpy(), index_param=f"IVF{NLIST},Flat", measurement="ip", nprobe=16)
torch.cuda.synchronize()
t0 = time.perf_counter()
ivf.train()
torch.cuda.synchronize()
train_s = time.perf_counter() - t0
flat = FaissSearcher(items=ivf.items[:8], index_param="Flat", measurement="ip")
flat.index = ivf.index  # the same device matrix


def ev(searcher):
    for qb in batches[:WARM]:
        searcher.search_index(qb, K)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for qb in batches[WARM:]:
        searcher.search_index(qb, K)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / args.reps


lens = (ivf.list_off[1:] - ivf.list_off[:-1]).float()
res = {"shape": {"queries": B, "items": N, "dim": E, "k": K, "nlist": NLIST, "niter": ivf.niter},
       "train_s": round(train_s, 3),
       "list_len": {"min": int(lens.min().item()), "mean": round(lens.mean().item(), 1), "max": int(lens.max().item())},
       "flat_ms": round(ev(flat), 3), "ivf": []}
flat_i = flat.search_index(batches[WARM], K)[1]
for nprobe in args.nprobe:
    ivf.nprobe = nprobe
    ms = ev(ivf)
    got = ivf.search_index(batches[WARM], K)[1]
    hit = torch.cat([(got[r:r + 128].unsqueeze(2) == flat_i[r:r + 128].unsqueeze(1)).any(dim=2).float().mean(dim=1)
                     for r in range(0, B, 128)])
    res["ivf"].append({"nprobe": nprobe, "ms": round(ms, 3), "recall_at_200": round(hit.mean().item(), 4),
                       "speedup_vs_flat": round(res["flat_ms"] / ms, 2)})
print(json.dumps(res))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
