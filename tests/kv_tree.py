"""What the token-tree tests share (tests/test_kvtree_cpu.py, tests/test_gpu_kvtree.py): the visibility rule of
flash_attention_n_kvcache_tree as a boolean [B, 1, Sq, S] builder, the depth rule, the mask builders, the operand builders of the C ABI
over fake pointers, the fp32 reference per batch element and the runner. A plain module: no tests, importable without a GPU.

The rule (kvcache.py's docstring). qlen_b = clamp(query_seqlens[b], 0, Sq), len_b the cache length the forward sees, base_b = len_b -
qlen_b. Node i < qlen_b sees key j iff
    0 <= j < base_b (under a window W also j > p_i - W), or j = base_b + t with 0 <= t < qlen_b and bit t of word (b, i) set,
p_i = base_b + d_i, d_i = max(popcount(word & low qlen_b bits) - 1, 0). Positions i >= qlen_b see nothing."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_args as ka   # noqa: E402
import kv_support as ks   # noqa: E402

FULL = (1 << 64) - 1


# ---------------------------------------------------------------- words
def signed(w):
    """an unsigned 64-bit word as the int64 a tensor holds (bit 63 is the sign bit)"""
    w &= FULL
    return w - (1 << 64) if w >> 63 else w


def words_tensor(rows, dev="cpu"):
    """[B][Sq] Python words -> int64 [B, Sq]"""
    return torch.tensor([[signed(w) for w in row] for row in rows], dtype=torch.int64, device=dev)


def words_of(masks):
    """int64 [B, Sq] -> [B][Sq] unsigned Python words"""
    return [[w & FULL for w in row] for row in masks.cpu().tolist()]


def depth(word, qlen):
    """max(popcount(word & low qlen bits) - 1, 0)"""
    return max(bin(word & FULL & ((1 << qlen) - 1)).count("1") - 1, 0)


def depths(masks, qlens):
    """int64 [B, Sq] of the depths (padding nodes: 0)"""
    rows = words_of(masks)
    return torch.tensor([[depth(w, ql) if i < ql else 0 for i, w in enumerate(row)] for row, ql in zip(rows, qlens)], dtype=torch.int64)


# ---------------------------------------------------------------- mask builders: one row of Sq words each
def chain(Sq):
    """bit t iff t <= i: causal attention"""
    return [(1 << (i + 1)) - 1 for i in range(Sq)]


def random_tree(Sq, gen):
    """a random parent among the earlier nodes; a row is the ancestor closure plus the node itself. Returns (words, parents)"""
    words, parents = [], []
    for i in range(Sq):
        par = -1 if i == 0 else int(torch.randint(0, i, (1,), generator=gen))
        parents.append(par)
        words.append((1 << i) | (words[par] if par >= 0 else 0))
    return words, parents


def star(Sq):
    """the node itself plus the root"""
    return [(1 << i) | 1 for i in range(Sq)]


def arbitrary(Sq, gen):
    """random 64-bit words - upper-triangular bits, bits beyond Sq, missing self bits - with at least one all-zero row and, at Sq = 64,
    bit 63 set in some rows (a key) and node 63 seeing something (a node)"""
    hi = torch.randint(0, 1 << 32, (Sq,), generator=gen).tolist()
    lo = torch.randint(0, 1 << 32, (Sq,), generator=gen).tolist()
    words = [(h << 32) | l for h, l in zip(hi, lo)]
    words[Sq // 2] = 0
    if Sq == 64:
        words[3] |= 1 << 63
        words[63] |= (1 << 63) | 1
        words[5] &= ~(1 << 63) & FULL
    return words


# ---------------------------------------------------------------- the rule
def tree_vis(lens, qlens, Sq, S, masks, window=None, dev="cpu"):
    """[B, 1, Sq, S] bool of the rule above; `lens`: len_b as the forward sees it"""
    B = len(lens)
    m = masks.to("cpu")
    ln = torch.tensor(lens).view(B, 1, 1)
    ql = torch.tensor(qlens).view(B, 1, 1)
    base = ln - ql
    i = torch.arange(Sq).view(1, Sq, 1)
    j = torch.arange(S).view(1, 1, S)
    tb = torch.arange(64).view(1, 1, 64)
    bits = (((m.unsqueeze(-1) >> tb) & 1) != 0) & (tb < ql)                      # [B, Sq, 64]: node i sees node t, valid nodes only
    p = base + (bits.sum(-1, keepdim=True) - 1).clamp_min(0)                      # [B, Sq, 1]
    prefix = (j < base) & (j >= 0)
    if window is not None:
        prefix = prefix & (j > p - window)
    t = j - base                                                                  # [B, 1, S]
    new = (t >= 0) & (t < ql) & torch.gather(bits, 2, t.clamp(0, 63).expand(B, Sq, S))
    return ((prefix | new) & (i < ql)).view(B, 1, Sq, S).to(dev)


def tree_vis_brute(len_b, qlen_b, S, words, window=None):
    """[qlen_b, S] bool of one batch element, one key at a time in Python integers"""
    base = len_b - qlen_b
    vis = torch.zeros(qlen_b, S, dtype=torch.bool)
    for i in range(qlen_b):
        p = base + depth(words[i], qlen_b)
        for j in range(S):
            if j < base:
                vis[i, j] = window is None or j > p - window
            else:
                t = j - base
                vis[i, j] = t < qlen_b and bool((words[i] >> t) & 1)
    return vis


def reference_tree(q, kg, vg, lens, qlens, n, masks, window=None, scale=None):
    """kv_support.reference per batch element on q[b, :, :qlen_b] under the tree rule; padding positions: 0 / -inf"""
    B, H, Sq, D = q.shape
    dev = q.device
    S = kg.shape[2]
    o = torch.zeros(B, H, Sq, D, dtype=torch.float32, device=dev)
    lse = torch.full((B, H, Sq), float("-inf"), dtype=torch.float32, device=dev)
    nb = ks._bh(torch.as_tensor(n, dtype=torch.float32, device=dev), B, H)
    vis = tree_vis(lens, qlens, Sq, S, masks, window, dev)
    for b in range(B):
        ql = qlens[b]
        if ql == 0:
            continue
        ob, lb = ks.reference(q[b:b + 1, :, :ql], kg[b:b + 1], vg[b:b + 1], vis[b:b + 1, :, :ql], nb[b:b + 1], None, scale)
        o[b, :, :ql] = ob[0]
        lse[b, :, :ql] = lb[0]
    return o, lse


# ---------------------------------------------------------------- operands of the C ABI (fake pointers: plans and validation only)
def _tree(pkg, window=0, reserved=0, mask=ka.DUMMY + 1024, stride=64):
    return pkg._lib.KvTree(mask=mask, batch_stride=stride, window=window, reserved=reserved)


def _commit(pkg, B=2, Hkv=2, D=64, page=64, max_pages=4, A=4, nodes=16, paged=True, **over):
    c = pkg._lib.KvTreeCommit()
    c.k_cache = c.v_cache = ka.DUMMY
    for i, s in enumerate((page * Hkv * D, Hkv * D, D)):
        c.k_stride[i] = c.v_stride[i] = s
    c.block_table = ka.DUMMY if paged else None
    c.block_table_stride, c.max_pages, c.page_size = max_pages, max_pages, page
    c.seqlens, c.B, c.Hkv, c.D, c.A = ka.DUMMY, B, Hkv, D, A
    c.accepted, c.accepted_stride, c.accepted_lens, c.nodes, c.reserved = ka.DUMMY + 256, A, ka.DUMMY + 512, nodes, 0
    for k, v in over.items():
        setattr(c, k, v)
    return c


# shapes whose tree plans are recorded (tests/golden/kvtree_plans.txt): a 16-node and a 64-node tree on both routes, a short and a long cache
DECODE_CASES = {
    "gqa16": dict(B=4, H=64, Hkv=8, Sq=16, D=64, page=256, max_pages=32),
    "mha64": dict(B=64, H=16, Hkv=16, Sq=64, D=128, page=256, max_pages=32),
    "one": dict(B=1, H=8, Hkv=1, Sq=16, D=64, page=64, max_pages=64),
}
PREFILL_CASES = {
    "gqa40": dict(B=3, H=8, Hkv=1, Sq=40, D=64, page=64, max_pages=8),
    "g4_64": dict(B=2, H=16, Hkv=4, Sq=64, D=64, page=256, max_pages=32),
    "long": dict(B=1, H=64, Hkv=8, Sq=64, D=64, page=256, max_pages=128),
}
GOLDEN_WINDOWS = (0, 128, 1000)


# ---------------------------------------------------------------- the runner (GPU)
def run_tree(pkg, dev, H, Hkv, Sq, D, dtype, page, prefix, rows, n, qlens=None, append=False, window=None, seed=1, max_pages=None, what="",
             scale=None, poison=False):
    """One tree call on a freshly built paged cache against reference_tree, under kv_support's gates. `prefix`: base_b per batch element;
    `rows`: [B][Sq] words; `append`: the nodes' K/V rows come as k_new / v_new (otherwise they are in the cache already); `poison`
    (window): every row and table entry wholly below first_b is poisoned first. Returns (out, lse, o_ref, lse_ref)."""
    B = len(prefix)
    ql = [Sq] * B if qlens is None else list(qlens)
    total = [p + x for p, x in zip(prefix, ql)]
    max_pages = max_pages or max(1, max((t + page - 1) // page for t in total)) + 1
    Smax = page * max_pages
    q = ks._rand((B, H, Sq, D), dtype, dev, seed)
    kd = ks._rand((B, Hkv, Smax, D), dtype, dev, seed + 1)
    vd = ks._rand((B, Hkv, Smax, D), dtype, dev, seed + 2, std=1.0)
    masks = words_tensor(rows, dev)
    kn = vn = None
    if append:
        pc = ks._Paged(kd, vd, prefix, page, max_pages, seed, alloc_all=True)
        kn, vn = (torch.zeros(B, Hkv, Sq, D, dtype=dtype, device=dev) for _ in range(2))
        for b in range(B):
            kn[b, :, :ql[b]], vn[b, :, :ql[b]] = kd[b, :, prefix[b]:total[b]], vd[b, :, prefix[b]:total[b]]
    else:
        pc = ks._Paged(kd, vd, total, page, max_pages, seed)
    kg, vg = ks._visible_dense(kd, total), ks._visible_dense(vd, total)
    if poison:
        assert window is not None
        assert ks._poison(pc.k, pc.v, pc.table, page, pc.poison, total, ql, window) > 0
    qs = None if qlens is None else torch.tensor(ql, dtype=torch.int32, device=dev)
    out, lse = pkg.flash_attention_n_kvcache_tree(q, pc.k, pc.v, pc.lens, masks, block_table=pc.table, k_new=kn, v_new=vn, query_seqlens=qs,
                                                  softmax_n_param=n, scale=scale, return_lse=True, window=window)
    if not poison:   # the cache the forward saw, read back through the table: the dense picture, appended rows included
        assert torch.equal(ks._bits(ks._gather(pc.k, pc.table, total, page)), ks._bits(kg[:, :, :max(1, max((t + page - 1) // page for t in total)) * page]))
    o_ref, lse_ref = reference_tree(q, kg, vg, total, ql, n, masks, window, scale)
    ks._check(out, o_ref, dtype, f"{what} out")
    ks._check_lse(lse, lse_ref, f"{what} lse")
    for b in range(B):
        assert (out[b, :, ql[b]:] == 0).all() and (lse[b, :, ql[b]:] == float("-inf")).all(), f"{what}: padding rows of batch element {b}"
    return out, lse, o_ref, lse_ref
