"""What the K/V-cache layout tests share (tests/test_kvlayout_cpu.py, tests/test_gpu_kvlayout.py): the cache's layout contract - "any strided
view whose rows are 16-byte aligned with feature stride 1; never copied" - turned into operands. A plain module: no tests, importable
without a GPU.

  rehouse     the logical pools kv_support._Paged / kv_fp8.PagedCodes build ([P, page, Hkv, D], or dense [B, cap, Hkv, D]) in new storage
              under two layouts, so that K and V differ in ALL THREE strides:
                nhd_pad  storage [P, page + 1, Hkv + 1, D], view [:, :page, :Hkv]      row stride (Hkv + 1) D, padded page stride
                hnd      storage [P, Hkv, page, D], view .permute(0, 2, 1, 3)          row stride D, head stride page D (vLLM's HND)
              L1 = K nhd_pad, V hnd; L2 = K hnd, V nhd_pad. Storage outside a view is a gap and holds a sentinel bit pattern that no test
              value and no stale row uses: a NaN with a payload in the 16-bit types (stale rows are the default NaN), 0xff for codes
              (stale code rows are 0x7f). gaps_intact compares the integer bits of everything outside the view with it.
  far_ids     three page ids of ONE contiguous pool of about 4.5 GiB, [P, 2, page, Hkv, D] serving K and V: for both, the byte offsets of
              the three pages lie below 2^31, in [2^31, 2^32) and at or above 2^32; and the pages an offset that wrapped at 2^31 or 2^32
              would hit instead (the aliases), which with the neighbours of the used pages carry the sentinel.
  operand views  query / k_new / v_new, padded and token-packed, with k_new and v_new differing in stride, each 16-byte aligned so that
              kvcache._rows hands the very tensor to the kernels (no_copy asserts it); block_table, tree_mask and accepted as slices of
              wider tensors.
  gather / scatter  a cache read and written on the CPU through (strides, table) and nothing else - the address arithmetic of the
              kernels in plain integers - with the mutants the CPU suite shows the GPU checks would catch.
  recording   the launch plans and the strides of the argument blocks of the calls made inside it; dry_run: the same with the launches
              taken out, over CPU tensors - the host layer's checks, blocks and plans without a device.
  ROUTES      one case per compiled forward text and per writing kernel, with what builds its operands (_setup, _operands), makes its call
              (_invoke) and checks plans and the fp64 gate of tests/kv_witness.py (_check_plans, _check_reference)."""
import contextlib
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_fp8 as k8         # noqa: E402
import kv_fp8_tree as k8t   # noqa: E402
import kv_support as ks     # noqa: E402
import kv_tree as kt        # noqa: E402
import kv_witness as kw     # noqa: E402

F8 = torch.float8_e4m3fn
SENTINEL = {torch.bfloat16: 0x7FA5, torch.float16: 0x7DA5, F8: 0xFF, torch.uint8: 0xFF}   # NaN with a payload; torch's own NaN is 0x7fc0 / 0x7e00
LAYOUTS = {"L1": ("nhd_pad", "hnd"), "L2": ("hnd", "nhd_pad")}
NAN = float("nan")


def ints(t):
    """the integer bits of a 16-bit or one-byte tensor (a view)"""
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.uint8)


def house(t, kind, sentinel=None):
    """one logical pool [P, page, Hkv, D] in new storage of layout `kind`: (the view in t's dtype, the storage as integers)"""
    P, page, Hkv, D = t.shape
    bits = ints(t)
    s = SENTINEL[t.dtype] if sentinel is None else sentinel
    if kind == "nhd_pad":
        store = torch.full((P, page + 1, Hkv + 1, D), s, dtype=bits.dtype, device=t.device)
        view = store[:, :page, :Hkv]
    else:
        assert kind == "hnd"
        store = torch.full((P, Hkv, page, D), s, dtype=bits.dtype, device=t.device)
        view = store.permute(0, 2, 1, 3)
    view.copy_(bits)
    return view.view(t.dtype), store


def rehouse(k, v, layout, *, sentinel=None):
    """(k view, v view, k storage, v storage) of the logical pools under L1 / L2. The views hold the pools' bits, are not contiguous,
    differ in page, row and head stride and are caches kvcache._check_cache accepts."""
    from flash_attention_softmax_n_amd import kvcache
    kk, vk = LAYOUTS[layout]
    kv, kst = house(k, kk, sentinel)
    vv, vst = house(v, vk, sentinel)
    assert kv.shape == k.shape and vv.shape == v.shape and torch.equal(ints(kv), ints(k)) and torch.equal(ints(vv), ints(v))
    assert all(kv.stride(i) != vv.stride(i) for i in range(3)), (kv.stride(), vv.stride())
    assert kv.stride(3) == vv.stride(3) == 1 and not kv.is_contiguous() and not vv.is_contiguous()
    for name, t in (("k_cache", kv), ("v_cache", vv)):
        kvcache._check_cache(name, t, True, t.shape[3])
    return kv, vv, kst, vst


def expected_strides(kind, page, Hkv, D):
    """(page, row, head) element strides of a view of layout `kind`"""
    return ((page + 1) * (Hkv + 1) * D, (Hkv + 1) * D, D) if kind == "nhd_pad" else (Hkv * page * D, D, page * D)


def gaps_intact(storage, view, sentinel=None):
    """True iff every element of `storage` outside `view` still holds the sentinel (integer bits compared)"""
    s = SENTINEL[view.dtype] if sentinel is None else sentinel
    inside = torch.zeros(storage.numel(), dtype=torch.bool, device=storage.device)
    torch.as_strided(inside, tuple(view.shape), tuple(view.stride()), view.storage_offset() - storage.storage_offset()).fill_(True)
    return bool((storage.reshape(-1)[~inside] == s).all())


# ---------------------------------------------------------------- the far pool
FAR_BYTES = 9 << 29   # 4.5 GiB


def far_ids(page_bytes, pool_bytes=FAR_BYTES):
    """The far pool [P, 2, page, Hkv, D]: page p of K starts at byte p * slot, of V at p * slot + page_bytes, slot = 2 * page_bytes.
    Returns dict(pages=P, slot, ids=(lo, mid, hi), k_off, v_off (byte offsets of the three pages), aliases (the pages the offsets taken
    mod 2^31 and mod 2^32 touch), guard (aliases and the neighbours of the used pages: what holds the sentinel))."""
    slot = 2 * page_bytes
    P = pool_bytes // slot
    at = lambda limit: -(-limit // slot)   # noqa: E731  the first page at or beyond a byte offset
    ids = (P // 64 + 7, at(1 << 31) + 11, at(1 << 32) + 13)
    k_off = tuple(p * slot for p in ids)
    v_off = tuple(p * slot + page_bytes for p in ids)
    assert ids[2] + 1 < P
    for off in (k_off, v_off):
        assert off[0] + page_bytes <= 1 << 31 and 1 << 31 <= off[1] and off[1] + page_bytes <= 1 << 32 and 1 << 32 <= off[2]
    aliases = set()
    for off in k_off + v_off:
        for mod in (1 << 31, 1 << 32):
            if off >= mod:
                a = off % mod
                aliases.update((a // slot, (a + page_bytes - 1) // slot))
    guard = (aliases | {p + d for p in ids for d in (-1, 1)}) - set(ids)
    assert not aliases & set(ids) and len(set(ids)) == 3
    return dict(pages=P, slot=slot, ids=ids, k_off=k_off, v_off=v_off, aliases=sorted(aliases), guard=sorted(guard))


def far_pool(like, dev):
    """The far pool for pages shaped like those of the logical pool `like` ([*, page, Hkv, D]): uninitialised integer storage
    [P, 2, page, Hkv, D] whose guard pages hold the sentinel, the K and V views in like's dtype, and far_ids' dict."""
    _, page, Hkv, D = like.shape
    info = far_ids(page * Hkv * D * like.element_size())
    store = torch.empty((info["pages"], 2, page, Hkv, D), dtype=ints(like).dtype, device=dev)
    for g in info["guard"]:
        store[g] = SENTINEL[like.dtype]
    return store, store[:, 0].view(like.dtype), store[:, 1].view(like.dtype), info


def far_guard_intact(store, info, dtype):
    return all(bool((store[g] == SENTINEL[dtype]).all()) for g in info["guard"])


# ---------------------------------------------------------------- operand views
def no_copy(t4):
    """a [B, heads, S, D] operand view reaches the kernels as it is: kvcache._rows makes no contiguous copy of it"""
    from flash_attention_softmax_n_amd import kvcache
    assert kvcache._rows(t4) is t4 and not t4.is_contiguous(), tuple(t4.stride())
    return t4


def q_view(q):
    """[B, H, Sq, D] as the transpose of [B, Sq, H, D] storage"""
    return no_copy(q.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3))


def k_new_view(t):
    """[B, Hkv, Sq, D] permuted from [B, Sq, Hkv, D] storage"""
    return no_copy(t.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3))


def v_new_view(t):
    """[B, Hkv, Sq, D] as a slice of a padded [B, Hkv, Sq + 1, D] (NaN in the padding): strides unlike k_new_view's"""
    B, Hkv, Sq, D = t.shape
    store = torch.full((B, Hkv, Sq + 1, D), NAN, dtype=t.dtype, device=t.device)
    store[:, :, :Sq] = t
    return no_copy(store[:, :, :Sq])


def packed_views(q, kn=None, vn=None, Hkv=None):
    """token-packed [T, H, D] / [T, Hkv, D]: query and k_new sliced from one fused [T, (H + 2 Hkv) D] buffer, v_new from
    [T, Hkv + 1, D][:, :Hkv]; NaN wherever no operand lies"""
    T, H, D = q.shape
    Hkv = kn.shape[1] if kn is not None else Hkv
    fused = torch.full((T, (H + 2 * Hkv) * D), NAN, dtype=q.dtype, device=q.device)
    fused[:, :H * D] = q.reshape(T, -1)
    qv = fused[:, :H * D].unflatten(1, (H, D))
    no_copy(qv.unsqueeze(0).transpose(1, 2))
    if kn is None:
        return qv, None, None
    fused[:, H * D:(H + Hkv) * D] = kn.reshape(T, -1)
    knv = fused[:, H * D:(H + Hkv) * D].unflatten(1, (Hkv, D))
    vstore = torch.full((T, Hkv + 1, D), NAN, dtype=vn.dtype, device=vn.device)
    vstore[:, :Hkv] = vn
    vnv = vstore[:, :Hkv]
    for t in (knv, vnv):
        no_copy(t.unsqueeze(0).transpose(1, 2))
    assert knv.stride() != vnv.stride()
    return qv, knv, vnv


def column_slice(t, fill, left=2, right=1):
    """a 2-D argument (block_table, tree_mask, accepted) as a column slice of a wider tensor: row stride > its width"""
    wide = torch.full((t.shape[0], left + t.shape[1] + right), fill, dtype=t.dtype, device=t.device)
    wide[:, left:left + t.shape[1]] = t
    view = wide[:, left:left + t.shape[1]]
    assert view.stride(0) > t.shape[1] and view.stride(1) == 1 and torch.equal(view, t)
    return view


# ---------------------------------------------------------------- a cache through (strides, table) on the CPU
def offsets(strides, table, page, Hkv, B, S, base=0, wrap=None):
    """element offsets [B, Hkv, S] of feature 0 of key j of head h of sequence b: base + table[b][j // page] * ps + (j % page) * rs + h * hs
    (table None: a dense cache, page = b). `wrap`: the offset taken mod `wrap` elements - an address formed in too few bits."""
    ps, rs, hs = strides
    j = torch.arange(S, dtype=torch.int64)
    pid = torch.arange(B, dtype=torch.int64).view(B, 1).expand(B, S) if table is None else table.long()[:, j // page]
    off = base + (pid * ps + (j % page).view(1, S) * rs).view(B, 1, S) + (torch.arange(Hkv, dtype=torch.int64) * hs).view(1, Hkv, 1)
    return off if wrap is None else off % wrap


def gather(storage, strides, table, page, Hkv, D, B, S, base=0):
    """dense [B, Hkv, S, D] read from the flat storage through (strides, table); None where an offset leaves the storage (a fault)"""
    flat = storage.reshape(-1)
    idx = offsets(strides, table, page, Hkv, B, S, base).unsqueeze(-1) + torch.arange(D)
    if idx.min() < 0 or idx.max() >= flat.numel():
        return None
    return flat[idx]


def scatter(storage, rows, strides, table, page, lens, base=0, row_shift=0):
    """rows [B, Hkv, Sq, D] (integer bits) written at the keys lens[b] + i + row_shift of the flat storage through (strides, table)"""
    B, Hkv, Sq, D = rows.shape
    flat = storage.reshape(-1)
    ps, rs, hs = strides
    for b in range(B):
        for i in range(Sq):
            key = lens[b] + i
            pid = b if table is None else int(table[b, key // page])
            for h in range(Hkv):
                off = base + pid * ps + (key % page + row_shift) * rs + h * hs
                if off < 0 or off + D > flat.numel():
                    raise IndexError(f"offset {off} leaves the storage")
                flat[off:off + D] = rows[b, h, i]


# ---------------------------------------------------------------- what a call launched
@contextlib.contextmanager
def recording(pkg, launch=True):
    """Inside: every K/V-cache call appends to the yielded list (entry point, its launch plan or None where the ABI has no plan for it,
    the (k_stride, v_stride) of its argument block). The plans are asked of the library for the very blocks the call launches."""
    kc, L = pkg.kvcache, pkg._lib
    rec, fwd, app = [], kc._forward, kc._append

    def strides(c):
        return tuple(c.kv.k_stride), tuple(c.kv.v_stride)

    def forward(lib, c, stream, win=None, tree=None, fp8=None):
        _, _, name, plan, ops = L.kv_forward_call(c.stem, fp8=fp8, tree=tree, window=win, alibi=c.alibi)
        rec.append((name, L._kv_plan(plan, c.args, *ops), strides(c)))
        return fwd(lib, c, stream, win, tree, fp8) if launch else None

    def append(lib, c, stream, rope=None, q_rot=None, tree=None, fp8=None):
        if rope is not None or c.k_new is not None:
            name, ops = L.kv_append_call(c.stem, fp8=fp8, tree=tree, rope=rope)
            plan = None
            if hasattr(lib, name + "_plan"):
                views = [None if t is None else kc._view4(t) for t in (c.k_new, c.v_new)]
                plan = L._kv_plan(name + "_plan", c.args, *ops, kc._view4(q_rot), *views)
            rec.append((name, plan, strides(c)))
        if launch:
            return app(lib, c, stream, rope, q_rot, tree, fp8)
        if rope is not None:   # (what the launch leaves behind: the forward reads the rotated queries)
            c.kv.q = kc._view4(q_rot)

    kc._forward, kc._append = forward, append
    try:
        yield rec
    finally:
        kc._forward, kc._append = fwd, app


def kernels(rec):
    """the kernel names (template arguments dropped) a recorded call launched, entry points without a plan by their own name"""
    out = []
    for name, plan, _ in rec:
        out += [name] if plan is None else [k[0].split("<")[0] for k in plan]
    return out


# ---------------------------------------------------------------- the routes: one per compiled forward text and per writing kernel
H, HKV = 8, 2
LENS, QL40, TAIL = [0, 61, 130], [40, 7, 0], 7
W = 40   # the window of the longest sequence starts at first_b = 64: a tile inside a page of 256, and a page of 64 the server has freed
PACKED = dict(lens=[0, 61, 120, 60], qlens=[1, 0, 16, 17], Sq=17)   # the appends of sequences 2 and 3 cross a page and a tile edge
BF16, FP16 = torch.bfloat16, torch.float16

# call: the entry point; Sq / qlens decide between the decode and the prefill kernels; `fwd` / `writer`: the kernels the plan must name
ROUTES = {
    "decode": dict(call="decode", Sq=3, append=True, fwd="fasn_kvcache_fwd_kernel", writer="fasn_kvcache_append"),
    "decode_alibi": dict(call="decode", Sq=3, alibi=True, fwd="fasn_kvcache_fwd_alibi_kernel"),
    "decode_window": dict(call="window", Sq=3, window=W, append=True, fwd="fasn_kvcache_fwd_window_kernel", writer="fasn_kvcache_append"),
    "decode_tree": dict(call="tree", Sq=13, tree=True, append=True, fwd="fasn_kvcache_fwd_tree_kernel", writer="fasn_kvcache_append"),
    "prefill": dict(call="prefill", Sq=40, qlens=QL40, append=True, fwd="fasn_kvprefill_fwd_kernel", writer="fasn_kvprefill_append"),
    "prefill_alibi": dict(call="prefill", Sq=40, qlens=QL40, alibi=True, fwd="fasn_kvprefill_fwd_alibi_kernel"),
    "prefill_window": dict(call="window", Sq=40, qlens=QL40, window=W, append=True, fwd="fasn_kvprefill_fwd_window_kernel",
                           writer="fasn_kvprefill_append"),
    "prefill_tree": dict(call="tree", Sq=13, qlens=[13, 7, 0], tree=True, append=True, fwd="fasn_kvprefill_fwd_tree_kernel",
                         writer="fasn_kvprefill_append"),
    "packed": dict(call="varlen", packed=True, append=True, fwd="fasn_kvvarlen_fwd_kernel", writer="fasn_kvvarlen_append", **PACKED),
    "packed_window": dict(call="varlen_window", packed=True, window=W, append=True, fwd="fasn_kvvarlen_fwd_window_kernel",
                          writer="fasn_kvvarlen_append", **PACKED),
    "rope_decode": dict(call="rope", Sq=3, rope=True, append=True, fwd="fasn_kvcache_fwd_kernel", writer="fasn_kvrope_kernel"),
    "rope_prefill": dict(call="rope", Sq=40, qlens=QL40, rope=True, append=True, fwd="fasn_kvprefill_fwd_kernel", writer="fasn_kvrope_kernel"),
    "rope_packed": dict(call="varlen_rope", packed=True, rope=True, append=True, fwd="fasn_kvvarlen_fwd_kernel", writer="fasn_kvvarlen_rope_kernel",
                        **PACKED),
    "rope_tree": dict(call="tree", Sq=13, tree=True, rope=True, append=True, fwd="fasn_kvcache_fwd_tree_kernel",
                      writer="fasn_kvcache_tree_rope_append"),
    "fp8_decode": dict(call="fp8", Sq=3, fp8=True, append=True, fwd="fasn_kvcache_fwd_fp8_kernel", writer="fasn_kvcache_fp8_append"),
    "fp8_prefill": dict(call="fp8", Sq=40, qlens=QL40, fp8=True, append=True, fwd="fasn_kvprefill_fwd_fp8_kernel", writer="fasn_kvprefill_fp8_append"),
    "fp8_window_decode": dict(call="fp8_window", Sq=3, window=W, fp8=True, append=True, fwd="fasn_kvcache_fwd_fp8_window_kernel",
                              writer="fasn_kvcache_fp8_append"),
    "fp8_window_prefill": dict(call="fp8_window", Sq=40, qlens=QL40, window=W, fp8=True, append=True, fwd="fasn_kvprefill_fwd_fp8_window_kernel",
                               writer="fasn_kvprefill_fp8_append"),
    "fp8_tree_decode": dict(call="fp8_tree", Sq=13, tree=True, fp8=True, append=True, fwd="fasn_kvcache_fwd_fp8_tree_kernel",
                            writer="fasn_kvcache_fp8_append"),
    "fp8_tree_prefill": dict(call="fp8_tree", Sq=13, qlens=[13, 7, 0], tree=True, fp8=True, append=True, fwd="fasn_kvprefill_fwd_fp8_tree_kernel",
                             writer="fasn_kvprefill_fp8_append"),
    "fp8_rope_decode": dict(call="fp8_rope", Sq=3, rope=True, fp8=True, append=True, fwd="fasn_kvcache_fwd_fp8_kernel", writer="fasn_kvrope_fp8_kernel"),
    "fp8_rope_prefill": dict(call="fp8_rope", Sq=40, qlens=QL40, rope=True, fp8=True, append=True, fwd="fasn_kvprefill_fwd_fp8_kernel",
                             writer="fasn_kvrope_fp8_kernel"),
    "fp8_tree_rope": dict(call="fp8_tree", Sq=13, tree=True, rope=True, fp8=True, append=True, fwd="fasn_kvcache_fwd_fp8_tree_kernel",
                          writer="fasn_kvrope_fp8_tree_kernel"),
}


# ---------------------------------------------------------------- one case: operands, the dense picture, the pools
def _setup(dev, route, dtype, D, page, seed, lens=None, max_pages=None, dense=False, qlens=None):
    """One case of a route on `dev` (the CPU serves the suite without a GPU): kv_witness.inputs_c at logit std 4, the tree words, the
    eager rotation, the dense picture AFTER the call in the cache's own numbers (k_exp / v_exp) and widened (k_eff / v_eff: the operands
    of the fp64 reference, with q_eff), k_new / v_new, and the logical pools BEFORE the call with every row the call is to write stale."""
    r = ROUTES[route]
    lens = list(lens or r.get("lens") or LENS)
    B = len(lens)
    qlens = qlens or r.get("qlens")
    if qlens is not None and len(qlens) != B:   # (a case of one sequence)
        qlens = qlens[:B]
    case = kw.Case(r["call"], H, HKV, D, r["Sq"], lens, page=page, max_pages=max_pages, qlens=qlens, window=r.get("window"),
                   append=r.get("append", False), alibi=r.get("alibi", False))
    inp = kw.inputs_c(case, 4, dtype, dev, seed)
    ql, total, cap, Sq = case.qlens, case.total, case.cap, case.Sq
    s = types.SimpleNamespace(r=r, route=route, case=case, dtype=dtype, D=D, page=page, dev=dev, B=B, dense=dense, fp8=bool(r.get("fp8")),
                              packed=bool(r.get("packed")), scale=inp["scale"], n=inp["n"], slopes=inp.get("slopes"),
                              qs=None if qlens is None or r.get("packed") else torch.tensor(ql, dtype=torch.int32, device=dev))
    s.rows = s.masks = None
    step = torch.arange(Sq).view(1, Sq).expand(B, Sq)
    if r.get("tree"):
        gen = torch.Generator().manual_seed(seed)
        s.rows = [kt.random_tree(Sq, gen)[0] for _ in range(B)]
        s.masks = kt.words_tensor(s.rows, dev)
        step = kt.depths(s.masks, ql)
    q, kd, vd = inp["q"], inp["kd"].clone(), inp["vd"]
    kn, vn = kw._new_rows(case, inp)
    s.cos = s.sin = None
    if r.get("rope"):   # rotate the queries and the new keys in eager torch: node / position i of k_new at lens_b + step, of q at base_b + step
        s.cos, s.sin = ks._tables(cap, D, dev, torch.float32)
        q_eff = ks._rotate(q, torch.tensor(total).view(B, 1) - torch.tensor(ql).view(B, 1) + step, s.cos, s.sin, False)
        k_rot = ks._rotate(kn, torch.tensor(lens).view(B, 1) + step, s.cos, s.sin, False)
        for b in range(B):
            kd[b, :, lens[b]:lens[b] + ql[b]] = k_rot[b, :, :ql[b]]
    else:
        q_eff = q
    s.q, s.q_eff, s.kn, s.vn = q, q_eff, kn, vn
    if s.fp8:   # the cache holds the codes of the dense picture; k_new / v_new are values the append quantises back to exactly those codes
        s.ksc, s.vsc = k8.scales_bh(k8.POW2_SCALES, B, HKV, dev, seed + 7), k8.scales_bh(k8.POW2_SCALES, B, HKV, dev, seed + 8)
        kcode, vcode = k8.quantise(kd, s.ksc[:, :, None, None]).to(dev), k8.quantise(vd, s.vsc[:, :, None, None]).to(dev)
        s.k_eff, s.v_eff = k8.up(kcode).double() * s.ksc[:, :, None, None].double(), k8.up(vcode).double() * s.vsc[:, :, None, None].double()
        if case.append:
            new = lambda code, sc: torch.stack([(k8.up(code[b, :, lens[b]:lens[b] + Sq]) * sc[b, :, None, None]).to(dtype) for b in range(B)])   # noqa: E731
            s.vn = _pad_rows(new(vcode, s.vsc), ql)
            if not r.get("rope"):
                s.kn = _pad_rows(new(kcode, s.ksc), ql)
        s.k_exp, s.v_exp = kcode, vcode
        pc = k8.PagedCodes(kcode, vcode, total, page, case.max_pages, seed)
        for b in range(B):   # the rows the call is to write are stale before it
            for pos in range(lens[b], total[b]):
                pc.ku[int(pc.table[b, pos // page]), pos % page] = pc.vu[int(pc.table[b, pos // page]), pos % page] = k8.NAN_CODE
        if case.window is not None:   # rows and table entries wholly below the window's first tile are gone
            k8t.poison_below(pc, total, ql, case.window)
        s.k_pool, s.v_pool, s.table, s.poison = pc.k, pc.v, pc.table, pc.poison
    else:
        s.k_eff, s.v_eff, s.k_exp, s.v_exp = kd.double(), vd.double(), kd, vd
        if dense:
            s.k_pool, s.v_pool = (torch.full((B, cap, HKV, D), NAN, dtype=dtype, device=dev) for _ in range(2))
            for b in range(B):
                s.k_pool[b, :lens[b]], s.v_pool[b, :lens[b]] = kd[b, :, :lens[b]].transpose(0, 1), vd[b, :, :lens[b]].transpose(0, 1)
            s.table = None
        else:
            pc = kw._cache(case, dict(inp, kd=kd), seed)
            s.k_pool, s.v_pool, s.table, s.poison = pc.k, pc.v, pc.table, pc.poison
    s.lens_t = torch.tensor(lens, dtype=torch.int32, device=dev)
    return s


def _pad_rows(t, ql):
    """[B, Hkv, Sq, D] with the rows at or beyond qlen_b zeroed (kv_witness._new_rows' padding)"""
    for b, x in enumerate(ql):
        t[b, :, x:] = 0
    return t


def _pack(s, t):
    """[B, heads, Sq, D] -> token-packed [T, heads, D] with TAIL rows of NaN behind cu[B]"""
    rows = [t[b, :, :x].transpose(0, 1) for b, x in enumerate(s.case.qlens)]
    return torch.cat(rows + [torch.full((TAIL, t.shape[1], t.shape[3]), NAN, dtype=t.dtype, device=t.device)], 0).contiguous()


def _operands(s, k, v, table, strided):
    """the operand set of one call: on the views of kv_layout when `strided`, contiguous otherwise"""
    o = types.SimpleNamespace(k=k, v=v, lens=s.lens_t, table=table, masks=s.masks, kn=None, vn=None)
    if s.packed:
        q, kn, vn = _pack(s, s.q), _pack(s, s.kn), _pack(s, s.vn)
        o.q, o.kn, o.vn = packed_views(q, kn, vn) if strided else (q, kn, vn)
        o.cu, o.maxq = ks._cu(s.case.qlens, s.dev), max(s.case.qlens)
    else:
        o.q = q_view(s.q) if strided else s.q.contiguous()
        if s.case.append:
            o.kn, o.vn = (k_new_view(s.kn), v_new_view(s.vn)) if strided else (s.kn.contiguous(), s.vn.contiguous())
            assert not strided or o.kn.stride() != o.vn.stride()
    if strided:
        if table is not None:
            o.table = column_slice(table, s.poison)
        if s.masks is not None:
            o.masks = column_slice(s.masks, -1)
    return o


def _invoke(pkg, s, o):
    r, call = s.r, s.r["call"]
    kw_ = dict(block_table=o.table, k_new=o.kn, v_new=o.vn, softmax_n_param=s.n, scale=s.scale, return_lse=True)
    if not s.packed and call != "decode":
        kw_["query_seqlens"] = s.qs
    if call in ("rope", "varlen_rope", "fp8_rope") or (r.get("tree") and r.get("rope")):
        kw_.update(rotary_cos=s.cos, rotary_sin=s.sin)
    pre = (o.q, o.k, o.v, o.lens)
    if call == "decode":
        return pkg.flash_attention_n_kvcache(*pre, alibi_slopes=s.slopes, **kw_)
    if call == "prefill":
        return pkg.flash_attention_n_kvcache_prefill(*pre, alibi_slopes=s.slopes, **kw_)
    if call == "window":
        return pkg.flash_attention_n_kvcache_window(*pre, r["window"], **kw_)
    if call == "tree":
        return pkg.flash_attention_n_kvcache_tree(*pre, o.masks, **kw_)
    if call == "rope":
        return pkg.flash_attention_n_kvcache_rope(*pre, **kw_)
    if call == "varlen":
        return pkg.flash_attention_n_kvcache_varlen(*pre, o.cu, o.maxq, **kw_)
    if call == "varlen_window":
        return pkg.flash_attention_n_kvcache_varlen_window(*pre, o.cu, o.maxq, r["window"], **kw_)
    if call == "varlen_rope":
        return pkg.flash_attention_n_kvcache_varlen_rope(*pre, o.cu, o.maxq, **kw_)
    if call == "fp8":
        return pkg.flash_attention_n_kvcache_fp8(*pre, s.ksc, s.vsc, **kw_)
    if call == "fp8_window":
        return pkg.flash_attention_n_kvcache_fp8_window(*pre, s.ksc, s.vsc, r["window"], **kw_)
    if call == "fp8_rope":
        return pkg.flash_attention_n_kvcache_fp8_rope(*pre, s.ksc, s.vsc, **kw_)
    assert call == "fp8_tree"
    return pkg.flash_attention_n_kvcache_fp8_tree(*pre, s.ksc, s.vsc, o.masks, **kw_)


def _per_sequence(s, out, lse):
    """per sequence (out [H, qlen_b, D], lse [H, qlen_b]); padding rows of the prefill kernels exactly 0 / -inf"""
    if not s.packed:
        return kw._rows_of(s.case, out, lse, s.qs is not None)
    res, t0 = [], 0
    for x in s.case.qlens:
        res.append((out[t0:t0 + x].transpose(0, 1), lse[:, t0:t0 + x]))
        t0 += x
    return res


def _written(s, out, lse):
    """the part of the outputs a call defines (a packed call leaves the rows behind cu[B] unwritten)"""
    used = sum(s.case.qlens)
    return (out[:used], lse[:, :used]) if s.packed else (out, lse)


def _live(s, S, dev):
    """[B, 1, S, 1] bool: the rows first_b <= j < len_b of the cache after the call - those a window's memory contract keeps (no window:
    first_b = 0)"""
    W = s.case.window
    first = [ks._first(t, x, W) if W is not None else 0 for t, x in zip(s.case.total, s.case.qlens)]
    j = torch.arange(S, device=dev).view(1, 1, -1, 1)
    return (j < torch.tensor(s.case.total, device=dev).view(-1, 1, 1, 1)) & (j >= torch.tensor(first, device=dev).view(-1, 1, 1, 1))


def _logical(s, pool, table, page):
    """integer bits [B, Hkv, S, D] of the live rows of the cache after the call, read through the table (every other row: 0)"""
    bits = ints(pool)
    if table is None:
        d = bits.permute(0, 2, 1, 3)
    else:
        need = max(1, max((t + page - 1) // page for t in s.case.total))
        d = bits[table[:, :need].long()].reshape(s.B, need * page, HKV, s.D).permute(0, 2, 1, 3)
    return torch.where(_live(s, d.shape[2], pool.device), d, torch.zeros_like(d))


def _dense_bits(s, exp):
    """integer bits of the dense picture [B, Hkv, cap, D] with every row but the live ones zeroed"""
    return torch.where(_live(s, exp.shape[2], exp.device), ints(exp), torch.zeros_like(ints(exp)))


def _check_reference(s, got, what):
    """(e): the fp64 gate of kv_witness on the strided call's own outputs"""
    case, ratios = s.case, []
    f = lambda t: t.detach().to("cpu", torch.float64)   # noqa: E731
    n = f(s.n)
    for b in range(s.B):
        ln, x = case.total[b], case.qlens[b]
        if s.rows is not None:
            w = kt.tree_vis_brute(ln, x, ln, s.rows[b], case.window).double()
        else:
            w = kw.visible(ln, x, ln, True, case.window).double()
        bias = None if s.slopes is None else kw.alibi_bias(f(s.slopes), ln, x, ln)
        ref = kw.attend(f(s.q_eff[b, :, :x]), f(s.k_eff[b, :, :ln]), f(s.v_eff[b, :, :ln]), w, n, s.scale, bias)
        ratios.append(kw.gate_c(got[b][0], ref, s.dtype))
        ks._check_lse(got[b][1], ref["lse"], f"{what} sequence {b} lse")
    print(f"{what}: out at {max(ratios):.3g} of 3 u A + 1e-6")
    assert max(ratios) <= 1, f"{what}: out is {max(ratios):.3g}x (3 u A + 1e-6) from the fp64 reference, per sequence {ratios}"


def _check_plans(s, rec_s, rec_c, k, v, what):
    """(d), the strides the blocks carried, and the kernels the route is there to reach"""
    assert [(n, p) for n, p, _ in rec_s] == [(n, p) for n, p, _ in rec_c], f"{what}: strides changed the plan: {rec_s} / {rec_c}"
    want = tuple(tuple(t.stride(i) if t.size(i) > 1 else 0 for i in range(3)) for t in (k, v))
    assert all(st == want for _, _, st in rec_s), f"{what}: the argument blocks carry {[st for _, _, st in rec_s]}, the views have {want}"
    names = kernels(rec_s)
    print(f"{what}: kernels {names}")
    assert s.r["fwd"] in names and (s.r.get("writer") is None or s.r["writer"] in names) and bool(s.r.get("writer")) == bool(s.case.append), names


# ---------------------------------------------------------------- the host layer without a device
class _OnDevice(torch.Tensor):
    """a CPU tensor that says it lives on the device: kvcache._prepare then fills its argument block from it (nothing is dereferenced)"""
    is_cuda = property(lambda self: True)


def on_device(t):
    return t.as_subclass(_OnDevice)


@contextlib.contextmanager
def dry_run(pkg):
    """recording() with the launches taken out: the calls inside check their operands, fill their argument blocks and ask the library
    for the launch plans of those very blocks - over CPU tensors whose addresses are never dereferenced, as tests/kv_args.py's fake
    pointers are not. The outputs of a call are uninitialised. `query` (and a commit's k_cache) must be on_device()."""
    kc = pkg.kvcache
    saved = kc._on_device, kc._stream_ptr
    kc._on_device, kc._stream_ptr = (lambda dev, launch: launch()), (lambda dev: None)
    try:
        with recording(pkg, launch=False) as rec:
            yield rec
    finally:
        kc._on_device, kc._stream_ptr = saved
