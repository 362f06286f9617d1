"""What the MLA tests share. Without a GPU: the error codes and builders of the C ABI's argument blocks and operands over fake, aligned
pointers (nothing built here is ever dereferenced). On the GPU: the shapes, the paged latent cache, the fp32 torch references of the dense
and the sparse decode, the index lists and the split counts read from the launch plans. A plain module: no tests, importable without a GPU."""
import functools

import torch

from kv_support import _bh, _gather, _n_values, _Paged, _rand, _visibility

EINVAL, EDTYPE, EHEADDIM, EALIGN, ESTRIDE, EUNSUPPORTED = -1, -2, -3, -4, -5, -7
BASE = 1 << 20

E, EV = 576, 512
SCALE = (128 + 64) ** -0.5
LENS = [0, 1, 63, 64, 65, 129, 1100]   # empty, shorter than Sq, a tile edge from both sides, a page edge, a length that is split


# ---------------------------------------------------------------- argument blocks and operands (no GPU)
def _args(pkg, **over):
    """a block every check accepts: B = 2, H = 16, Sq = 2, page 64 x 4 pages, bf16 (pointers are never dereferenced)"""
    a = pkg._lib.MlaArgs()
    base = 1 << 20
    a.q.ptr = a.o.ptr = a.kv_cache = a.seqlens = a.block_table = base
    for v, d in ((a.q, 576), (a.o, 512)):
        v.stride[0], v.stride[1], v.stride[2], v.stride[3] = 16 * 2 * d, 2 * d, d, 1
    a.kv_stride[0], a.kv_stride[1] = 64 * 576, 576
    a.block_table_stride, a.max_pages, a.page_size = 4, 4, 64
    a.B, a.H, a.Sq, a.D, a.Dv, a.dtype = 2, 16, 2, 576, 512, 1
    a.scale, a.softmax_n, a.causal = 192 ** -0.5, 1.0, 1
    for k, v in over.items():
        obj, _, leaf = k.rpartition(".")
        tgt = getattr(a, obj) if obj else a
        if leaf.startswith("stride"):
            tgt.stride[int(leaf[6:])] = v
        else:
            setattr(tgt, leaf, v)
    return a


def _fp8(pkg, **over):
    f = pkg._lib.MlaFp8()
    f.kv_scale, f.sb, f.reserved = BASE, 1, 0
    for k, v in over.items():
        setattr(f, k, v)
    return f


def _sparse(pkg, **over):
    s = pkg._lib.MlaSparse()
    s.indices, s.stride_b, s.stride_q, s.topk, s.reserved = BASE, 2 * 2048, 2048, 2048, 0
    for k, v in over.items():
        setattr(s, k, v)
    return s


def _block(pkg, stride=(64 * 656, 656), **over):
    a = _args(pkg, **over)   # _args's block over 656-byte rows: kv_stride counts bytes
    a.kv_stride[0], a.kv_stride[1] = stride
    return a


def _index_args(pkg, **over):
    """a block every check accepts: B = 3, Hi = 64, Sq = 2, page 64 x 96 pages, bf16, topk 2048 (pointers are never dereferenced)"""
    a = pkg._lib.MlaIndexArgs()
    a.q.ptr = a.w = a.k_cache = a.seqlens = a.block_table = a.indices = BASE
    a.q.stride[0], a.q.stride[1], a.q.stride[2], a.q.stride[3] = 64 * 2 * 128, 2 * 128, 128, 1
    a.w_stride[0], a.w_stride[1], a.w_stride[2] = 128, 2, 1
    a.k_stride[0], a.k_stride[1] = 64 * 128, 128
    a.block_table_stride, a.max_pages, a.page_size = 96, 96, 64
    a.B, a.Hi, a.Sq, a.D, a.dtype, a.causal, a.topk = 3, 64, 2, 128, 1, 1, 2048
    a.indices_stride[0], a.indices_stride[1] = 2 * 2048, 2048
    a.logits_stride[0], a.logits_stride[1] = 2 * 6144, 6144
    for k, v in over.items():
        name, _, i = k.partition("#")
        tgt = a.q if name == "q.stride" else a
        if i:
            getattr(tgt, name.rpartition(".")[2])[int(i)] = v
        else:
            setattr(a, name, v)
    return a


# ---------------------------------------------------------------- the dense decode on the GPU
def _ref(q, rows, lens, n, causal, scale=SCALE):
    """rows: [B, S, 576] with the rows at or beyond len_b zeroed. Returns (out [B, H, Sq, 512], lse [B, H, Sq]) in fp32."""
    B, H, Sq, _ = q.shape
    x = scale * torch.einsum("bhqd,bsd->bhqs", q.float(), rows.float())
    x = x.masked_fill(~_visibility(lens, Sq, rows.shape[1], causal, q.device), float("-inf"))
    sink = _bh(torch.as_tensor(n, dtype=torch.float32, device=q.device), B, H).log()[..., None, None].expand(B, H, Sq, 1)   # (log 0 = -inf)
    xs = torch.cat([sink, x], -1)
    lse = torch.logsumexp(xs, -1)
    p = torch.exp(xs - torch.where(torch.isfinite(lse), lse, torch.zeros_like(lse))[..., None])[..., 1:]
    return torch.einsum("bhqs,bsd->bhqd", p, rows[..., :EV].float()), lse


@functools.lru_cache(maxsize=None)
def _cache(dtype, page, lens=tuple(LENS), alloc_all=False, seed=3):
    """one paged latent cache per (dtype, page): stale rows and unnamed pages are NaN (_Paged). Returns (pool, its gathered rows)."""
    dev = torch.device("cuda")
    max_pages = max(1, max((ln + page - 1) // page for ln in lens)) + 1
    rows = _rand((len(lens), 1, page * max_pages, E), dtype, dev, seed)
    pc = _Paged(rows, rows, list(lens), page, max_pages, seed, alloc_all=alloc_all)
    return pc, _gather(pc.k, pc.table, list(lens), page)[:, 0]


def _nsplit(pkg, B, H, Sq, page, max_pages, paged=True):
    a = pkg._lib.MlaArgs()
    a.q.ptr = a.o.ptr = a.kv_cache = a.seqlens = 1 << 20
    a.block_table = (1 << 20) if paged else None
    for v, d in ((a.q, E), (a.o, EV)):
        v.stride[0], v.stride[1], v.stride[2], v.stride[3] = H * Sq * d, Sq * d, d, 1
    a.kv_stride[0], a.kv_stride[1], a.block_table_stride, a.max_pages, a.page_size = page * E, E, max_pages, max_pages, page
    a.B, a.H, a.Sq, a.D, a.Dv, a.dtype, a.scale = B, H, Sq, E, EV, 1, SCALE
    fwd = pkg._lib.mla_plan(a)[0]
    return fwd[1] // (B * ((H * Sq + 63) // 64))


def _n(kind, B, H, dev):
    return _n_values((B, H), dev, 11) if kind == "tensor" else kind


# ---------------------------------------------------------------- the sparse decode on the GPU
def _entry_vis(idx, lens, Sq, causal):
    """[B, Sq, topk] bool: entry j is a key of position i iff 0 <= j < len_b and (causal) j <= i + len_b - Sq"""
    ln = torch.as_tensor(lens, device=idx.device).view(-1, 1, 1)
    vis = (idx >= 0) & (idx < ln)
    return vis & (idx <= torch.arange(Sq, device=idx.device).view(1, -1, 1) + ln - Sq) if causal else vis


def _ref_sparse(q, rows, idx, lens, n, causal):
    """rows: [B, S, 576], the cache read through the table. Returns (out [B, H, Sq, 512], lse [B, H, Sq], vis) in fp32."""
    B, H, Sq, _ = q.shape
    vis = _entry_vis(idx, lens, Sq, causal)
    g = rows.float()[torch.arange(B, device=q.device).view(-1, 1, 1), idx.clamp(0, rows.shape[1] - 1).long()]   # [B, Sq, topk, 576]
    x = (SCALE * torch.einsum("bhqd,bqtd->bhqt", q.float(), g)).masked_fill(~vis[:, None], float("-inf"))
    sink = _bh(torch.as_tensor(n, dtype=torch.float32, device=q.device), B, H).log()[..., None, None].expand(B, H, Sq, 1)
    xs = torch.cat([sink, x], -1)
    lse = torch.logsumexp(xs, -1)
    p = torch.exp(xs - torch.where(torch.isfinite(lse), lse, torch.zeros_like(lse))[..., None])[..., 1:]
    return torch.einsum("bhqt,bqtd->bhqd", p, g[..., :EV]), lse, vis


def _lists(B, Sq, topk, capacity, seed, longest=None):
    """seeded CPU lists from [-1, capacity): -1, beyond-length, causally hidden and duplicate entries all occur. topk = 2048: the second
    half is -1, tile 2 (between live tiles) is -1, and tile 0 of element `longest` = (b, len) is 64 distinct positions every row sees"""
    gen = torch.Generator().manual_seed(seed)
    idx = torch.randint(-1, capacity, (B, Sq, topk), generator=gen, dtype=torch.int32)
    if topk == 2048:
        idx[..., 1024:] = -1
        idx[..., 128:192] = -1
        if longest is not None:
            idx[longest[0], :, :64] = torch.randperm(longest[1] - Sq + 1, generator=gen)[:64].to(torch.int32)
    return idx


def _nsplit_sparse(pkg, B, H, Sq, topk, max_pages, page=64):
    a = _args(pkg, B=B, H=H, Sq=Sq, max_pages=max_pages, block_table_stride=max_pages, page_size=page, block_table=(1 << 20) if max_pages > 1 else None)
    s = pkg._lib.MlaSparse()
    s.indices, s.stride_b, s.stride_q, s.topk = 1 << 20, Sq * topk, topk, topk
    return pkg._lib.mla_sparse_plan(a, s)[0][1] // (B * Sq * ((H + 63) // 64))
