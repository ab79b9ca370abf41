"""FaissSearcher on the GPU: inner-product / cosine search, exact ("Flat") or IVF-Flat ("IVF{nlist},Flat")
(reference: backend/third_party_components/faiss_searcher.py:23-225, which wraps faiss.index_factory).

index_param is "Flat" or "IVF<nlist>,Flat" (parse_index_param; anything else, HNSW / PQ included, raises
NotImplementedError), measurement "ip" | "cos".

Flat: the item matrix stays resident in HBM (fp32, l2-normalised for "cos" like __normvec__ :104-105), each query
batch is scored block by block with the MFMA GEMM (rf_linear_fwd: queries . items_block^T, 32768 items per block)
and the running top-k is merged after every block (rf_topk_merge: radix select + bitonic merge, ties by smaller
item index).

IVF-Flat (fp32 only): train() clusters the items with spherical k-means (assignment = argmax of the inner product
with the centroids, ties to the smaller list id: rf_linear_fwd + rf_topk_merge at k = 1; inverted lists by a stable
counting sort: rf_ivf_build_lists; centroid = the l2-normalised mean of its list: rf_gather_rows + rf_ivf_list_mean;
`niter` rounds on at most max_points_per_centroid * nlist rows drawn with torch.randperm(seed)), then assigns every
item and keeps the item rows in list order (items_sorted) beside the catalog-order matrix (self.index, which callers
gather rows from: IVF costs a second copy of the vectors). search_index() picks each query's `nprobe` best lists
(the same two kernels at k = nprobe), plans one candidate row per query (the probed lists' items side by side: torch
ops and one host read of the widest row, so it cannot run inside a graph capture; the (query, list) pairs grouped by
list with rf_ivf_build_lists), scores the probed lists list-major with rf_ivf_scan_f32 (every list read
once for all the queries that probe it, exact fp32 scores) and reduces each row with rf_topk_merge_idx, so the
result has Flat's type and conventions: scores descending, ties to the smaller item index, (-inf, -1) where the
probed lists hold fewer than k items. nprobe >= nlist is the exact search. faiss's own sampling and RNG are not
reproduced, so the lists are not faiss's lists; the contract is the semantics above plus recall.
save_index() / load_index() keep the trained lists (never the vectors) in an .npz.

Screened form (round 5; fp32 index, E >= 256, E % 32 == 0, more than one block, not inside a graph capture): the
first block is scored and merged as above, its k-th best score per query is a threshold no item of the exact top-k
falls below (the k-th best over all items is at least the k-th best of any subset), and ONE launch over the other
N - 32768 items (rf_ip_candidates_f32: the same fp32 MFMA scores, no score matrix written) keeps every item at or
above it; one rf_topk_merge_idx over those candidates and the first block's top-k gives the result. Same scores,
same ties (item index), same top-k as the block loop; a query whose candidate list overflows `cap` sends the whole
batch back to the block loop (one host read of the counts). It removes the [B, N] score matrix's write and re-read
(2 x 4.3 GB at the cfg5 shapes). On long catalogs (more than 8 blocks, E % 64 == 0) the first 4 blocks are scored
exactly for the threshold (blocks 2-4 screened by block 1's k-th score) and the rest is screened on bf16 copies (rf_ip_candidates_bf16: a pair is kept when its
bf16 score is within the bf16 error bound C ||q|| ||v|| of the threshold), the kept pairs rescored exactly in
rf_linear_fwd's k order (rf_ip_rescore_f32: the same bits) before the merge: the result is still the block loop's,
bit for bit.

search() returns what the reference returns without an encoder: (item_list[indexes], directories) for
an int topK, {k: (items, sims)} for a list of topK (:178-204).
"""
from __future__ import annotations

import re
from typing import List, Optional, Sequence, Union

import numpy as np
import torch

from ...runtime import lib as L

BLOCK = 32768
SCREEN_CAP_MAX = 32768  # rf_topk_merge_idx's column limit
# bf16 screen: |<q~, v~> - <q, v>| <= (2u + u^2 + 2 gamma_K (1 + u)^2) sum |q_i v_i| <= C ||q|| ||v|| with u = 2^-8 (bf16
# round to nearest), gamma_K = K 2^-24 / (1 - K 2^-24) for the fp32 sums of both (K <= 1024): 0.00791 at K = 1024;
# C = 0.008 also covers the rounding of the two norms
SCREEN_BF16_C = 0.008
SCREEN_EXACT_BLOCKS = 4  # leading blocks scored exactly for the threshold before a bf16 screen
IVF_MAX_LISTS = 32768  # rf_ivf_build_lists' limit, and rf_topk_merge's column limit (the coarse step)
IVF_MAX_PROBES = 1024  # rf_topk_merge's k limit
IVF_ASSIGN_ROWS = 65536  # rows per assignment chunk: the score buffer stays at or below 65536 x nlist floats
IVF_CAND_BYTES = 1 << 30  # candidate buffers (value + index) of one query sub-batch
IVF_MERGE_COLS = 32768  # rf_topk_merge_idx's column limit

_IVF_RE = re.compile(r"ivf(\d+),\s*flat")


def parse_index_param(s):
    """("flat", None) for "Flat", ("ivf", nlist) for "IVF<nlist>,Flat" (case-insensitive, optional space after the
    comma); every other faiss factory string raises NotImplementedError."""
    text = str(s).lower()
    if text == "flat":
        return "flat", None
    m = _IVF_RE.fullmatch(text)
    if m:
        return "ivf", int(m.group(1))
    raise NotImplementedError(f"index_param {s!r}: only 'Flat' and 'IVF<nlist>,Flat' are implemented")


def validate_ivf_arrays(list_off, list_ids, ntotal: int, nlist: int) -> None:
    """Host check of a stored IVF partition (numpy only): list_off has nlist + 1 non-decreasing entries from 0 to
    ntotal, list_ids is a permutation of 0 .. ntotal-1. Raises ValueError otherwise."""
    off = np.asarray(list_off)
    ids = np.asarray(list_ids)
    if off.ndim != 1 or ids.ndim != 1 or off.dtype.kind not in "iu" or ids.dtype.kind not in "iu":
        raise ValueError("IVF index: list_off and list_ids must be 1-d integer arrays")
    off = off.astype(np.int64)
    ids = ids.astype(np.int64)
    if len(off) != nlist + 1:
        raise ValueError(f"IVF index: list_off has {len(off)} entries, expected nlist + 1 = {nlist + 1}")
    if off[0] != 0 or off[-1] != ntotal:
        raise ValueError(f"IVF index: list_off runs from {off[0]} to {off[-1]}, expected 0 to {ntotal}")
    if np.any(np.diff(off) < 0):
        raise ValueError("IVF index: list_off decreases")
    if len(ids) != ntotal:
        raise ValueError(f"IVF index: list_ids has {len(ids)} entries, expected {ntotal}")
    if ntotal and (ids.min() < 0 or ids.max() >= ntotal):
        raise ValueError("IVF index: list_ids holds an id outside [0, ntotal)")
    if not np.all(np.bincount(ids, minlength=ntotal) == 1):
        raise ValueError("IVF index: list_ids is not a permutation (duplicate id)")


class FaissSearcher:
    def __init__(self, encoder=None, items=None, item_list: Optional[Sequence] = None, index_param: str = None,
                 measurement: Union[str, int] = None, norm_vec: bool = False, use_gpu: bool = True,
                 dtype=torch.float32, device="cuda", nprobe: int = 1, niter: int = 10, seed: int = 1234,
                 max_points_per_centroid: int = 256, **kwargs):
        if encoder is not None:
            raise NotImplementedError("FaissSearcher(encoder=...) (text encoders) is outside the hot path; pass vectors")
        if items is None or index_param is None or measurement is None:
            raise AssertionError("Args 'items' 'index_param' 'measurement' must be given.")
        items = items.detach().cpu().numpy() if isinstance(items, torch.Tensor) else items
        if not isinstance(items, np.ndarray):
            raise ReferenceError("如果不传入encoder，则item只能输入numpy.array类型")
        if len(items.shape) != 2:
            raise AssertionError(f"encoder=None, 输入只能是二维矩阵[(n, dim)]，当前维度为[{items.shape}]")
        if item_list is not None:
            assert len(item_list) == len(items), f"len(item_list)={len(item_list)} != len(items)={len(items)}"
        kind, nlist = parse_index_param(index_param)
        if measurement not in ("ip", "cos"):
            raise NotImplementedError(f"measurement {measurement!r}: only 'ip' and 'cos' are implemented")
        if kind == "ivf":
            if not 1 <= nlist <= IVF_MAX_LISTS:
                raise ValueError(f"index_param {index_param!r}: nlist must be in [1, {IVF_MAX_LISTS}]")
            if nprobe < 1:
                raise ValueError(f"nprobe must be at least 1, got {nprobe}")
            if niter < 0:
                raise ValueError(f"niter must not be negative, got {niter}")
            if max_points_per_centroid < 1:
                raise ValueError(f"max_points_per_centroid must be at least 1, got {max_points_per_centroid}")
            if dtype != torch.float32:
                raise NotImplementedError(f"IVF index with dtype {dtype}: only torch.float32 is implemented")
        L.load()
        L.require_gpu()
        self.kind, self.nlist = kind, nlist
        self.nprobe, self.niter, self.seed, self.max_points_per_centroid = nprobe, niter, seed, max_points_per_centroid
        self._centroids = self.list_off = self.list_ids = self.items_sorted = None
        self.index_param, self.measurement = index_param, measurement
        self.norm_vec = True if measurement == "cos" else norm_vec
        self.items = items
        self.item_list = np.array(item_list if item_list is not None else np.arange(len(items)))
        self.vec_dim = items.shape[1]
        self.dtype = dtype
        self.device = torch.device(device)
        self.index = None

    def get_vecs(self, items) -> torch.Tensor:
        x = items if isinstance(items, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(items))
        x = x.to(self.device, torch.float32)
        if self.norm_vec:
            x = x / (x * x).sum(dim=1, keepdim=True).sqrt()
        return x.to(self.dtype).contiguous()

    def train(self):
        """Flat: upload the item matrix. IVF: also cluster it (module docstring) and keep the rows in list order;
        self.index stays the [N, E] matrix in catalog order (callers gather rows from it), so an IVF index holds the
        vectors twice."""
        self.index = self.get_vecs(self.items)  # [N, E] resident in HBM
        if self.kind == "ivf":
            self._train_ivf()
        return self

    # ---- IVF-Flat ------------------------------------------------------------------------------------------------
    @property
    def centroids(self):
        """[nlist, E] fp32 on the device (None before train() / load_index())."""
        return None if self._centroids is None else self._centroids[:, :self.vec_dim]

    def _pad4(self, x: torch.Tensor) -> torch.Tensor:
        # E to a multiple of 4 with zero columns (16-byte rows for the kernels); changes no inner product
        pad = -x.shape[1] % 4
        return x if pad == 0 else torch.nn.functional.pad(x, (0, pad)).contiguous()

    def _gather(self, table: torch.Tensor, rows: torch.Tensor) -> torch.Tensor:
        out = torch.empty((rows.numel(), table.shape[1]), dtype=torch.float32, device=self.device)
        L.call("rf_gather_rows", L.ptr(rows), rows.numel(), L.ptr(table), L.DT_F32, table.shape[0], table.shape[1],
               L.ptr(out), L.stream_ptr())
        return out

    def _top_lists(self, x: torch.Tensor, k: int) -> torch.Tensor:
        """[rows, k] int64: each row's k best lists by inner product with the centroids, best first, ties to the
        smaller list id (k = 1: the k-means assignment)."""
        n, nlist, st = x.shape[0], self.nlist, L.stream_ptr()
        out_i = torch.empty((n, k), dtype=torch.int64, device=self.device)
        rows = min(n, IVF_ASSIGN_ROWS)
        scores = torch.empty((rows, nlist), dtype=torch.float32, device=self.device)
        out_v = torch.empty((rows, k), dtype=torch.float32, device=self.device)
        for r0 in range(0, n, IVF_ASSIGN_ROWS):
            m = min(IVF_ASSIGN_ROWS, n - r0)
            xs = x[r0:r0 + m]
            L.call("rf_linear_fwd", L.ptr(xs), L.DT_F32, m, x.shape[1], x.stride(0), L.ptr(self._centroids), nlist, None, 0,
                   L.ptr(scores), nlist, st)
            L.call("rf_topk_merge", L.ptr(scores), nlist, m, nlist, k, 0, None, None, 0, k, L.ptr(out_v), L.ptr(out_i[r0:]),
                   k, st)
        return out_i

    def _build_lists(self, assign: torch.Tensor):
        n = assign.numel()
        list_off = torch.empty(self.nlist + 1, dtype=torch.int32, device=self.device)
        list_ids = torch.empty(n, dtype=torch.int32, device=self.device)  # item indices (< 2^31) as uint32
        ws = L.workspace("rf_ivf_build_ws_bytes", self.device, n, self.nlist)
        L.call("rf_ivf_build_lists", L.ptr(assign), n, self.nlist, L.ptr(list_off), L.ptr(list_ids), L.ptr(ws), ws.numel(),
               L.stream_ptr())
        return list_off, list_ids

    def _assign(self, x: torch.Tensor) -> torch.Tensor:
        # a row of NaN scores has no best list (-1): list 0, so that the lists stay a partition
        return self._top_lists(x, 1).view(-1).clamp_(min=0).to(torch.int32)

    def _train_ivf(self):
        N, nlist = self.index.shape[0], self.nlist
        if nlist > N:
            raise ValueError(f"index_param {self.index_param!r}: nlist = {nlist} exceeds the {N} items")
        x = self._pad4(self.index)
        perm = torch.randperm(N, generator=torch.Generator().manual_seed(self.seed))
        nt = min(N, self.max_points_per_centroid * nlist)
        xt = self._gather(x, perm[:nt].to(self.device))  # the training rows
        self._centroids = xt[:nlist].clone()
        for _ in range(self.niter):
            off, ids = self._build_lists(self._assign(xt))
            rows = self._gather(xt, ids.to(torch.int64))
            L.call("rf_ivf_list_mean", L.ptr(rows), x.shape[1], L.ptr(off), nlist, 1, L.ptr(self._centroids), L.stream_ptr())
        self.list_off, self.list_ids = self._build_lists(self._assign(x))
        self.items_sorted = self._gather(x, self.list_ids.to(torch.int64))

    def _n_probe(self) -> int:
        if self.nprobe < 1:
            raise ValueError(f"nprobe must be at least 1, got {self.nprobe}")
        p = min(int(self.nprobe), self.nlist)
        if p > IVF_MAX_PROBES:
            raise ValueError(f"nprobe = {p} lists: at most {IVF_MAX_PROBES} lists can be probed")
        return p

    def search_probes(self, target) -> torch.Tensor:
        """[B, min(nprobe, nlist)] int64 on the device: the lists each query probes, best centroid first."""
        if self.kind != "ivf" or self._centroids is None:
            raise Exception("search_probes needs a trained IVF index")
        return self._top_lists(self._pad4(self.get_vecs(target)), self._n_probe())

    def _search_ivf(self, target, k: int):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("IVF search reads the candidate width on the host: it cannot run inside a graph capture")
        nprobe = self._n_probe()
        q = self._pad4(self.get_vecs(target))
        B, E = q.shape
        dev, st, nlist = self.device, L.stream_ptr(), self.nlist
        out_v = torch.full((B, k), -float("inf"), dtype=torch.float32, device=dev)
        out_i = torch.full((B, k), -1, dtype=torch.int64, device=dev)
        if B == 0:
            return out_v, out_i
        probes = self._top_lists(q, nprobe).clamp_(min=0)  # [B, nprobe]
        lens = (self.list_off[1:] - self.list_off[:-1]).to(torch.int64)[probes]  # [B, nprobe]
        ends = lens.cumsum(dim=1)
        col = (ends - lens).to(torch.int32)  # a pair's first column in its query's candidate row
        cap = int(ends[:, -1].max().item())  # the one host read
        if cap == 0:
            return out_v, out_i
        grp_list = torch.arange(nlist, dtype=torch.int32, device=dev)  # one group per list (empty where not probed)
        b_sub = max(1, IVF_CAND_BYTES // (cap * 8))
        for b0 in range(0, B, b_sub):
            bs = min(b_sub, B - b0)
            # the pairs (query-major, pair p = query p // nprobe) grouped by list: the same stable counting sort that
            # builds the inverted lists, with the pairs as items (its offsets are the groups' offsets)
            grp_off, order = self._build_lists(probes[b0:b0 + bs].reshape(-1).to(torch.int32))
            pair_q = torch.div(order, nprobe, rounding_mode="floor")
            pair_col = col[b0:b0 + bs].reshape(-1)[order]
            cand_v = torch.full((bs, cap), float("nan"), dtype=torch.float32, device=dev)
            cand_i = torch.empty((bs, cap), dtype=torch.int32, device=dev)
            qs = q[b0:b0 + bs]
            L.call("rf_ivf_scan_f32", L.ptr(qs), q.stride(0), bs, L.ptr(self.items_sorted), self.items_sorted.shape[0], E,
                   L.ptr(self.list_off), L.ptr(self.list_ids), L.ptr(grp_list), L.ptr(grp_off), nlist, L.ptr(pair_q),
                   L.ptr(pair_col), L.ptr(cand_v), L.ptr(cand_i), cap, st)
            # chained over column chunks: a chunk's output is the next one's prev (double-buffered, no aliasing)
            vals = [torch.empty((bs, k), dtype=torch.float32, device=dev) for _ in range(2)]
            idxs = [torch.empty((bs, k), dtype=torch.int64, device=dev) for _ in range(2)]
            cur, k_prev = 0, 0
            for c0 in range(0, cap, IVF_MERGE_COLS):
                n = min(IVF_MERGE_COLS, cap - c0)
                nxt = 1 - cur
                L.call("rf_topk_merge_idx", L.ptr(cand_v[:, c0:]), L.ptr(cand_i[:, c0:]), cap, bs, n, k, L.ptr(vals[cur]),
                       L.ptr(idxs[cur]), k_prev, k, L.ptr(vals[nxt]), L.ptr(idxs[nxt]), k, st)
                cur, k_prev = nxt, k
            out_v[b0:b0 + bs] = vals[cur]
            out_i[b0:b0 + bs] = idxs[cur]
        return out_v, out_i

    # ---- persistence ---------------------------------------------------------------------------------------------
    def save_index(self, index_save_path):
        """Write the trained index to an .npz (faiss.write_index, :206-207): the kind, vec_dim, ntotal and, for IVF,
        nlist, the centroids and the lists. Never the vectors (load_index takes them from `items`), no pickle."""
        if self.index is None:
            raise Exception("Faiss dose not train, please use train method before search or load a trained index...")
        data = {"kind": np.array(self.kind), "vec_dim": np.int64(self.vec_dim), "ntotal": np.int64(self.index.shape[0])}
        if self.kind == "ivf":
            data.update(nlist=np.int64(self.nlist), centroids=self.centroids.cpu().numpy(),
                        list_off=self.list_off.cpu().numpy().astype(np.int64),
                        list_ids=self.list_ids.cpu().numpy().astype(np.int64))
        with open(index_save_path, "wb") as f:
            np.savez(f, **data)

    def load_index(self, index_path):
        """Read an index written by save_index (faiss.read_index, :132-139) for this searcher's `items`: the file's
        kind, ntotal and dimension must match, and an IVF partition is checked on the host (validate_ivf_arrays)
        before anything is uploaded."""
        with np.load(index_path, allow_pickle=False) as f:
            data = {name: f[name] for name in f.files}
        kind, ntotal, dim = str(data["kind"]), int(data["ntotal"]), int(data["vec_dim"])
        assert kind == self.kind, f"Index kind {kind!r} != searcher kind {self.kind!r}"
        assert ntotal == len(self.items), f"Index sample nums {ntotal} != Items length {len(self.items)}"
        assert dim == self.vec_dim, f"Index dim {dim} != Vecs dim {self.vec_dim}"
        if kind == "ivf":
            nlist = int(data["nlist"])
            assert nlist == self.nlist, f"Index nlist {nlist} != searcher nlist {self.nlist}"
            cent = np.asarray(data["centroids"])
            if cent.shape != (nlist, dim) or cent.dtype != np.float32:
                raise ValueError(f"IVF index: centroids {cent.dtype}{cent.shape}, expected float32{(nlist, dim)}")
            validate_ivf_arrays(data["list_off"], data["list_ids"], ntotal, nlist)
        self.index = self.get_vecs(self.items)
        if kind == "ivf":
            self._centroids = self._pad4(torch.from_numpy(cent).to(self.device)).contiguous()
            self.list_off = torch.from_numpy(data["list_off"].astype(np.int32)).to(self.device)
            self.list_ids = torch.from_numpy(data["list_ids"].astype(np.int32)).to(self.device)
            self.items_sorted = self._gather(self._pad4(self.index), self.list_ids.to(torch.int64))
        return self

    @property
    def index(self):
        return self._index

    @index.setter
    def index(self, value):
        # assigning an index drops the bf16 screen's copy and the item norms derived from the old one
        self._index = value
        self._screen_key = None
        self.index_bf16 = self.index_norm = None

    def _bf16_screen_index(self):
        # keyed on the index tensor's identity and version as well: an in-place write to the index rebuilds them
        key = (self._index.data_ptr(), tuple(self._index.shape), self._index._version)
        if self.index_bf16 is None or self._screen_key != key:
            self.index_bf16 = self._index.to(torch.bfloat16).contiguous()
            self.index_norm = self._index.norm(dim=1).contiguous()
            self._screen_key = key
        return self.index_bf16, self.index_norm

    screen = True  # the screened search where it applies (A/B: False keeps the block loop)

    screen_bf16 = True  # the bf16 screen + exact rescoring where the catalog is long enough (A/B: False)

    def _screened(self, q: torch.Tensor, k: int):
        """The screened search (module docstring), or None when a candidate list overflowed."""
        B, E = q.shape
        N = self.index.shape[0]
        dev = self.device
        st = L.stream_ptr()
        bf = self.screen_bf16 and N > 2 * SCREEN_EXACT_BLOCKS * BLOCK and E % 64 == 0 and E <= 1024
        n0 = SCREEN_EXACT_BLOCKS * BLOCK if bf else BLOCK
        # the first block exactly (the block loop's scores and merge)
        scores = torch.empty((B, BLOCK), dtype=torch.float32, device=dev)
        v0 = torch.empty((B, k), dtype=torch.float32, device=dev)
        i0 = torch.empty((B, k), dtype=torch.int64, device=dev)
        L.call("rf_linear_fwd", L.ptr(q), L.DT_F32, B, E, q.stride(0), L.ptr(self.index), BLOCK, None, 0, L.ptr(scores),
               scores.stride(0), st)
        L.call("rf_topk_merge", L.ptr(scores), scores.stride(0), B, BLOCK, k, 0, None, None, 0, k, L.ptr(v0), L.ptr(i0), k, st)
        del scores
        lead_counts = []
        if n0 > BLOCK:
            # the next leading blocks exactly as well, but screened by the first block's k-th score (one fp32
            # compaction launch, one merge of its few candidates) instead of a score block and a merge each
            t0 = v0[:, k - 1].contiguous()
            cap0 = int(min(SCREEN_CAP_MAX, max(1024, 3 * k * (n0 - BLOCK) // BLOCK + k)))  # ~3x the expected count
            cnt0 = torch.zeros(B, dtype=torch.int32, device=dev)
            cv0 = torch.full((B, cap0), float("nan"), dtype=torch.float32, device=dev)
            ci0 = torch.empty((B, cap0), dtype=torch.int32, device=dev)
            L.call("rf_ip_candidates_f32", L.ptr(q), q.stride(0), B, L.ptr(self.index[BLOCK:]), n0 - BLOCK, E, L.ptr(t0),
                   cap0, L.ptr(cnt0), L.ptr(cv0), L.ptr(ci0), BLOCK, st)
            v1 = torch.empty_like(v0)
            i1 = torch.empty_like(i0)
            L.call("rf_topk_merge_idx", L.ptr(cv0), L.ptr(ci0), cap0, B, cap0, k, L.ptr(v0), L.ptr(i0), k, k, L.ptr(v1),
                   L.ptr(i1), k, st)
            v0, i0 = v1, i1
            lead_counts.append((cnt0, cap0))  # checked with the later counts (one host read)
        thr = v0[:, k - 1].contiguous()  # -inf where the blocks held fewer than k scores (then every item passes)
        # room for ~3x the candidates a uniform score distribution gives (k per n0 items; x1.5 for the bf16 margin)
        per = 3 * k * (N - n0) // n0 * (3 if bf else 2) // 2 + k
        cap = int(min(SCREEN_CAP_MAX, max(1024, per)))
        count = torch.zeros(B, dtype=torch.int32, device=dev)
        cval = torch.full((B, cap), float("nan"), dtype=torch.float32, device=dev)
        cidx = torch.empty((B, cap), dtype=torch.int32, device=dev)
        if bf:
            # candidates by bf16 scores within their error bound of the threshold, then their exact fp32 scores in
            # rf_linear_fwd's k order (rf_ip_rescore_f32: the same bits)
            ib, vn = self._bf16_screen_index()
            qb = q.to(torch.bfloat16).contiguous()
            qbound = (q.norm(dim=1) * SCREEN_BF16_C).contiguous()
            L.call("rf_ip_candidates_bf16", L.ptr(qb), qb.stride(0), B, L.ptr(ib[n0:]), N - n0, E, L.ptr(thr),
                   L.ptr(qbound), L.ptr(vn[n0:]), cap, L.ptr(count), L.ptr(cval), L.ptr(cidx), n0, st)
            if int(count.max().item()) > cap or any(int(c.max().item()) > cp for c, cp in lead_counts):
                return None
            L.call("rf_ip_rescore_f32", L.ptr(q), q.stride(0), B, L.ptr(self.index), E, L.ptr(count), cap, L.ptr(cval),
                   L.ptr(cidx), 0, st)
        else:
            L.call("rf_ip_candidates_f32", L.ptr(q), q.stride(0), B, L.ptr(self.index[n0:]), N - n0, E, L.ptr(thr), cap,
                   L.ptr(count), L.ptr(cval), L.ptr(cidx), n0, st)
            if int(count.max().item()) > cap:
                return None
        out_v = torch.empty((B, k), dtype=torch.float32, device=dev)
        out_i = torch.empty((B, k), dtype=torch.int64, device=dev)
        L.call("rf_topk_merge_idx", L.ptr(cval), L.ptr(cidx), cap, B, cap, k, L.ptr(v0), L.ptr(i0), k, k, L.ptr(out_v),
               L.ptr(out_i), k, st)
        return out_v, out_i

    def search_index(self, target, k: int):
        """(directories [B, k] fp32, indexes [B, k] int64) on the device — faiss index.search."""
        if self.index is None:
            raise Exception("Faiss dose not train, please use train method before search or load a trained index...")
        if not 1 <= k <= 1024:
            raise ValueError("topK must be in [1, 1024]")
        if self.kind == "ivf":
            return self._search_ivf(target, k)
        q = self.get_vecs(target)
        B, E = q.shape
        N = self.index.shape[0]
        if (self.screen and self.dtype == torch.float32 and N > BLOCK and E >= 256 and E % 32 == 0 and B > 0
                and not torch.cuda.is_current_stream_capturing()):
            res = self._screened(q, k)
            if res is not None:
                return res
        dev = self.device
        vals = [torch.empty((B, k), dtype=torch.float32, device=dev) for _ in range(2)]
        idxs = [torch.empty((B, k), dtype=torch.int64, device=dev) for _ in range(2)]
        scores = torch.empty((B, min(BLOCK, max(N, 1))), dtype=torch.float32, device=dev)
        st = L.stream_ptr()
        dt = L.torch_dtype_code(self.dtype)
        cur, k_prev = 0, 0
        for c0 in range(0, N, BLOCK):
            n = min(BLOCK, N - c0)
            blk = self.index[c0:c0 + n]
            L.call("rf_linear_fwd", L.ptr(q), dt, B, E, q.stride(0), L.ptr(blk), n, None, 0, L.ptr(scores), scores.stride(0), st)
            nxt = 1 - cur
            L.call("rf_topk_merge", L.ptr(scores), scores.stride(0), B, n, k, c0, L.ptr(vals[cur]), L.ptr(idxs[cur]), k_prev,
                   k, L.ptr(vals[nxt]), L.ptr(idxs[nxt]), k, st)
            cur, k_prev = nxt, k
        if k_prev == 0:
            vals[cur].fill_(-float("inf"))
            idxs[cur].fill_(-1)
        return vals[cur], idxs[cur]

    def search(self, target, topK: Union[int, List[int]], keep_rank_no=False):
        if isinstance(topK, int):
            d, i = self.search_index(target, topK)
            i = i.cpu().numpy()
            return (self.item_list[i], d.cpu().numpy(), i) if keep_rank_no else (self.item_list[i], d.cpu().numpy())
        if isinstance(topK, list):
            d, i = self.search_index(target, max(topK))
            d, i = d.cpu().numpy(), i.cpu().numpy()
            res = {}
            for k in topK:
                res[k] = (self.item_list[i[:, :k]], d[:, :k], i[:, :k]) if keep_rank_no else (self.item_list[i[:, :k]], d[:, :k])
            return res
        raise TypeError(f"TopK dose not support type: {type(topK)}")
