"""Token-tree attention over the K/V cache on the GPU: flash_attention_n_kvcache_tree and flash_attention_n_kvcache_tree_commit against the
fp32 reference of tests/kv_tree.py under kv_support's gates, bit for bit against the causal, window and rotary calls where the functions
coincide, and against the fp64 reference of tests/kv_witness.py where one key decides a row."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_args as ka   # noqa: E402
import kv_support as ks   # noqa: E402
import kv_tree as kt   # noqa: E402
import kv_witness as kw   # noqa: E402

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]
_ids = lambda d: str(d).split(".")[-1]   # noqa: E731


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rows(kind, Sq, B, seed):
    gen = _gen(seed)
    make = {"chain": lambda: kt.chain(Sq), "tree": lambda: kt.random_tree(Sq, gen)[0], "star": lambda: kt.star(Sq), "arbitrary": lambda: kt.arbitrary(Sq, gen)}[kind]
    return [make() for _ in range(B)]


def _nsplit_decode(pkg, dtype, window=0, **shape):
    plan = pkg._lib.kvtree_plan(ka._args_decode(pkg, dtype=1 if dtype == torch.bfloat16 else 0, **shape), kt._tree(pkg, window=window))
    assert [k[0].split("<")[0] for k in plan] == ["fasn_kvcache_fwd_tree_kernel", "fasn_kvcache_combine_kernel"]
    return plan[0][1] // (shape["B"] * shape["Hkv"])


def _prefill_names(pkg, dtype, window=0, **shape):
    plan = pkg._lib.kvtree_plan(ka._args_prefill(pkg, dtype=1 if dtype == torch.bfloat16 else 0, **shape), kt._tree(pkg, window=window))
    return [k[0].split("<")[0] for k in plan]


# ---------------------------------------------------------------- 1 - 3, 5, 6: geometry against the reference
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("kind", ["tree", "arbitrary"])
def test_tile_geometry_decode_route(pkg, dev, kind, dtype):
    """an empty prefix, a tree straddling a tile and page boundary, a tree starting on a boundary; n a tensor with zeros"""
    B, H, Hkv, Sq = 3, 8, 2, 13
    n = ks._n_values((B, H), dev, 5)
    assert (n == 0).any() and (n > 0).any()
    kt.run_tree(pkg, dev, H, Hkv, Sq, 64, dtype, 64, [0, 60, 128], _rows(kind, Sq, B, 7), n, seed=11, what=f"decode route {kind}")


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("kind", ["tree", "arbitrary"])
def test_prefill_route(pkg, dev, kind, dtype):
    """PB = 16: three row blocks, ragged query lengths with an empty one, the nodes appended"""
    B, H, Hkv, Sq = 3, 8, 1, 40
    assert _prefill_names(pkg, dtype, B=B, H=H, Hkv=Hkv, Sq=Sq, D=64, page=64, max_pages=5) == ["fasn_kvprefill_fwd_tree_kernel"]
    n = ks._n_values((B, H), dev, 6)
    kt.run_tree(pkg, dev, H, Hkv, Sq, 64, dtype, 64, [70, 0, 200], _rows(kind, Sq, B, 8), n, qlens=[40, 7, 0], append=True, seed=12, max_pages=5,
                what=f"prefill route {kind}")


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("G", [2, 4])
def test_full_word(pkg, dev, G, dtype):
    """Sq = 64: G = 2 is the decode route at 128 rows, G = 4 the prefill route; bit 63 as a key and as a node"""
    B, Hkv, Sq = 2, 2, 64
    rows = _rows("arbitrary", Sq, B, 9)
    assert all(r[63] >> 63 and any(w >> 63 for w in r[:63]) for r in rows)
    out, _lse, o_ref, _ = kt.run_tree(pkg, dev, G * Hkv, Hkv, Sq, 64, dtype, 64, [0, 61], rows, ks._n_values((G * Hkv,), dev, 4), seed=13,
                                      what=f"full word G={G}")
    # bit 63 matters: without it the reference of some row moves by more than the gate
    masks = kt.words_tensor([[w & ~(1 << 63) for w in r] for r in rows], dev)
    assert not torch.equal(kt.tree_vis([64, 125], [64, 64], 64, 128, masks), kt.tree_vis([64, 125], [64, 64], 64, 128, kt.words_tensor(rows)))


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_split_k(pkg, dev, dtype):
    """several splits, the tree's tiles in the last one; a star"""
    shape = dict(B=1, H=1, Hkv=1, Sq=16, D=64, page=64, max_pages=64)
    assert _nsplit_decode(pkg, dtype, **shape) > 1
    kt.run_tree(pkg, dev, 1, 1, 16, 64, dtype, 64, [3000], _rows("star", 16, 1, 1), 0.5, seed=14, max_pages=64, what="split-K star")


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("D", [32, 128, 256])
def test_outer_head_dims(pkg, dev, D, dtype):
    n = ks._n_values((4,), dev, 3)
    kt.run_tree(pkg, dev, 4, 2, 13, D, dtype, 64, [60, 131], _rows("tree", 13, 2, 21), n, seed=15, what=f"D={D} decode route")
    kt.run_tree(pkg, dev, 4, 1, 40, D, dtype, 64, [70, 3], _rows("tree", 40, 2, 22), n, qlens=[40, 9], append=True, seed=16, what=f"D={D} prefill route")


# ---------------------------------------------------------------- 4: the chain is causal attention, bit for bit
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_chain_equals_causal_bit_for_bit(pkg, dev, dtype):
    """Hidden scores are exact zeros in the sums and the split of the tiles is the base call's: equality is derived, not measured."""
    n = ks._n_values((8,), dev, 2)
    # decode route, several splits
    B, H, Hkv, Sq, page, mp = 2, 8, 2, 13, 64, 16
    assert _nsplit_decode(pkg, dtype, B=B, H=H, Hkv=Hkv, Sq=Sq, D=64, page=page, max_pages=mp) >= 2
    q, pc = ks._case(dev, B, H, Hkv, Sq, 64, dtype, page, [513, 143], 31, mp)
    masks = kt.words_tensor(_rows("chain", Sq, B, 0), dev)
    want = pkg.flash_attention_n_kvcache(q, pc.k, pc.v, pc.lens, block_table=pc.table, softmax_n_param=n, is_causal=True, return_lse=True)
    got = pkg.flash_attention_n_kvcache_tree(q, pc.k, pc.v, pc.lens, masks, block_table=pc.table, softmax_n_param=n, return_lse=True)
    assert torch.equal(ks._bits(got[0]), ks._bits(want[0])) and torch.equal(got[1], want[1])
    for W in (128, 64):   # (both hold all Sq nodes: a window never hides a node's ancestors)
        want = pkg.flash_attention_n_kvcache_window(q, pc.k, pc.v, pc.lens, W, block_table=pc.table, softmax_n_param=n, return_lse=True)
        got = pkg.flash_attention_n_kvcache_tree(q, pc.k, pc.v, pc.lens, masks, block_table=pc.table, softmax_n_param=n, return_lse=True, window=W)
        assert torch.equal(ks._bits(got[0]), ks._bits(want[0])) and torch.equal(got[1], want[1])
    # prefill route, one split in every plan
    B, H, Hkv, Sq, mp = 3, 8, 1, 40, 8
    shape = dict(B=B, H=H, Hkv=Hkv, Sq=Sq, D=64, page=page, max_pages=mp)
    assert _prefill_names(pkg, dtype, **shape) == ["fasn_kvprefill_fwd_tree_kernel"] == _prefill_names(pkg, dtype, window=128, **shape)
    assert ks._plan_names(pkg, dtype=1 if dtype == torch.bfloat16 else 0, **shape) == ["fasn_kvprefill_fwd_kernel"]
    q, pc = ks._case(dev, B, H, Hkv, Sq, 64, dtype, page, [110, 40, 300], 32, mp)
    masks = kt.words_tensor(_rows("chain", Sq, B, 0), dev)
    qs = torch.tensor([40, 40, 23], dtype=torch.int32, device=dev)
    for query_seqlens in (None, qs):
        want = pkg.flash_attention_n_kvcache_prefill(q, pc.k, pc.v, pc.lens, block_table=pc.table, softmax_n_param=n, is_causal=True, return_lse=True,
                                                     query_seqlens=query_seqlens)
        got = pkg.flash_attention_n_kvcache_tree(q, pc.k, pc.v, pc.lens, masks, block_table=pc.table, softmax_n_param=n, return_lse=True,
                                                 query_seqlens=query_seqlens)
        assert torch.equal(ks._bits(got[0]), ks._bits(want[0])) and torch.equal(got[1], want[1])
    want = pkg.flash_attention_n_kvcache_window(q, pc.k, pc.v, pc.lens, 128, block_table=pc.table, softmax_n_param=n, return_lse=True, query_seqlens=qs)
    got = pkg.flash_attention_n_kvcache_tree(q, pc.k, pc.v, pc.lens, masks, block_table=pc.table, softmax_n_param=n, return_lse=True, window=128,
                                             query_seqlens=qs)
    assert torch.equal(ks._bits(got[0]), ks._bits(want[0])) and torch.equal(got[1], want[1])


# ---------------------------------------------------------------- 7: window
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("route", ["decode", "prefill"])
def test_window(pkg, dev, route, dtype):
    """W = 128: every page wholly below first_b is NaN and its table entry names the poison page; a window at or beyond the capacity is no window"""
    prefix, W = [300, 100, 5000], 128
    H, Hkv, Sq, qlens = (8, 2, 13, None) if route == "decode" else (8, 1, 40, [40, 17, 33])
    rows = _rows("tree", Sq, 3, 17)
    n = ks._n_values((3, H), dev, 8)
    clean, lse_clean, _, _ = kt.run_tree(pkg, dev, H, Hkv, Sq, 64, dtype, 64, prefix, rows, n, qlens=qlens, window=W, seed=18, what=f"window {route}")
    dirty, lse_dirty, _, _ = kt.run_tree(pkg, dev, H, Hkv, Sq, 64, dtype, 64, prefix, rows, n, qlens=qlens, window=W, seed=18, poison=True,
                                         what=f"window {route} poisoned")
    assert torch.isfinite(dirty).all() and torch.equal(ks._bits(dirty), ks._bits(clean)) and torch.equal(lse_dirty, lse_clean)
    q, pc = ks._case(dev, 3, H, Hkv, Sq, 64, dtype, 64, [p + Sq for p in prefix], 19)
    masks = kt.words_tensor(rows, dev)
    none = pkg.flash_attention_n_kvcache_tree(q, pc.k, pc.v, pc.lens, masks, block_table=pc.table, softmax_n_param=n, return_lse=True)
    for Wbig in (pc.page * pc.max_pages, 2 ** 40):
        got = pkg.flash_attention_n_kvcache_tree(q, pc.k, pc.v, pc.lens, masks, block_table=pc.table, softmax_n_param=n, return_lse=True, window=Wbig)
        assert torch.equal(ks._bits(got[0]), ks._bits(none[0])) and torch.equal(got[1], none[1])


# ---------------------------------------------------------------- 8: one key decides
def _witness_run(pkg, case, inp, rows, seed):
    """the tree call on the witness's operands (no append: the nodes are cache rows already); per sequence (out, lse) and the fp64 reference"""
    dev = inp["q"].device
    pc = ks._Paged(inp["kd"], inp["vd"], case.total, case.page, case.max_pages, seed)
    out, lse = pkg.flash_attention_n_kvcache_tree(inp["q"], pc.k, pc.v, pc.lens, kt.words_tensor(rows, dev), block_table=pc.table,
                                                  softmax_n_param=inp["n"], scale=inp["scale"], return_lse=True)
    refs = []
    for b in range(case.B):
        q, k, v, n, _ = kw.sequence(case, inp, b)
        ln, ql = case.total[b], case.qlens[b]
        w = kt.tree_vis_brute(ln, ql, ln, rows[b]).double()
        refs.append((kw.attend(q, k[:, :ln], v[:, :ln], w, n, inp["scale"]), v[:, :ln]))
    return out, lse, refs


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("route", ["decode", "prefill"])
def test_witness_a_hidden_sibling_would_take_the_row(pkg, dev, route, dtype):
    """Form A. Node i's query is 64 e_s for a node s it does NOT see (a sibling where it has one), the key of node t is e_t, the prefix keys
    are 0 in those features: every visible logit is 0, the hidden key of s lies 64 nats above them. A leak of s replaces the row's
    output by V_s wholesale; the gate is witness C's, 3 u A + 1e-6 per element against fp64."""
    H, Hkv, Sq, D = (8, 2, 13, 64) if route == "decode" else (8, 1, 40, 64)
    prefix = [0, 60, 128]
    case = kw.Case(route, H, Hkv, D, Sq, [p + Sq for p in prefix])
    gen = _gen(23)
    trees = [kt.random_tree(Sq, gen) for _ in prefix]
    rows = [t[0] for t in trees]
    inp = dict(q=torch.zeros(case.B, H, Sq, D, dtype=dtype, device=dev), kd=ks._rand((case.B, Hkv, case.cap, D), dtype, dev, 41),
               vd=ks._rand((case.B, Hkv, case.cap, D), dtype, dev, 42, std=1.0), n=ks._n_values((H,), dev, 43), scale=1.0)
    inp["kd"][..., :Sq] = 0
    hidden = 0
    for b, (words, parents) in enumerate(trees):
        for i in range(Sq):
            sibs = [t for t in range(Sq) if t != i and parents[t] == parents[i]] or [t for t in range(Sq) if not (words[i] >> t) & 1]
            if sibs:
                s = sibs[int(torch.randint(0, len(sibs), (1,), generator=gen))]
                assert not (words[i] >> s) & 1
                inp["q"][b, :, i, s] = 64.0
                hidden += 1
            inp["kd"][b, :, prefix[b] + i, i] = 1.0
    assert hidden >= 3 * Sq - 3
    out, lse, refs = _witness_run(pkg, case, inp, rows, 44)
    for b, (ref, _v) in enumerate(refs):
        assert (ref["x"][torch.isfinite(ref["x"])] == 0).all()          # every visible logit is 0: the hidden one would be 64
        r = kw.gate_c(out[b], ref, dtype)
        print(f"witness A {route} sequence {b}: ratio {r:.3f}")
        assert r <= 1.0, (b, r)
        ks._check_lse(lse[b], ref["lse"].float(), f"witness A {route} lse {b}")


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("route", ["decode", "prefill"])
def test_witness_b_only_the_own_key(pkg, dev, route, dtype):
    """Form B. An empty prefix, every node sees its own key alone, q.k_j = j + 1 exactly and scale = 32 (kv_witness.inputs_b): the row is
    V_self / (1 + n 2^-x) with x >= 32 nats, V_self to two roundings (kv_witness.gate_b)."""
    H, Hkv, Sq, D = (8, 2, 13, 64) if route == "decode" else (8, 1, 40, 64)
    case = kw.Case(route, H, Hkv, D, Sq, [Sq, Sq])
    inp = kw.inputs_b(case, "ascending", dtype, dev, 51)
    rows = [[1 << i for i in range(Sq)] for _ in range(case.B)]
    out, _lse, refs = _witness_run(pkg, case, inp, rows, 52)
    for b, (ref, v) in enumerate(refs):
        kind, want = kw.expect_b(ref, v, H // Hkv)
        assert (kind == 1).all() and torch.equal(ref["x"].argmax(-1), torch.arange(Sq).expand(H, Sq))
        r = kw.gate_b(out[b], kind, want, dtype)
        print(f"witness B {route} sequence {b}: ratio {r:.3f}")
        assert r <= 1.0, (b, r)


# ---------------------------------------------------------------- 9: rotary at depth positions
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("route,interleaved,table32,rd", [("decode", False, True, 64), ("decode", True, False, 32), ("prefill", False, False, 48),
                                                          ("prefill", True, True, 64)])
def test_rotary_at_depth_positions(pkg, dev, route, interleaved, table32, rd, dtype):
    """The rows written are bit-equal to eager torch at positions base + depth; the output - a self-only batch element with n > 0 among
    them, where q decides the row through the sink's share - is bit-equal to the call without rotary on eagerly rotated operands; padding
    rows and rows beyond the capacity are untouched (whole-pool compare)."""
    H, Hkv, Sq, D, page, mp = (8, 2, 13, 64, 64, 3) if route == "decode" else (8, 1, 40, 64, 64, 3)
    B = 3
    prefix = [60, 0, page * mp - 5]                                      # the last one: all but 5 nodes fall beyond the capacity
    qlens = None if route == "decode" else [40, 7, 40]
    ql = [Sq] * B if qlens is None else qlens
    rows = _rows("tree", Sq, B, 61)
    rows[1] = [1 << i for i in range(Sq)]
    masks = kt.words_tensor(rows, dev)
    n = ks._n_values((B, H), dev, 62, zeros=False)
    q = ks._rand((B, H, Sq, D), dtype, dev, 63)
    kn, vn = ks._rand((B, Hkv, Sq, D), dtype, dev, 64), ks._rand((B, Hkv, Sq, D), dtype, dev, 65, std=1.0)
    cos, sin = ks._tables(page * mp, rd, dev, torch.float32 if table32 else dtype)
    kd, vd = ks._rand((B, Hkv, page * mp, D), dtype, dev, 66), ks._rand((B, Hkv, page * mp, D), dtype, dev, 67, std=1.0)
    qs = None if qlens is None else torch.tensor(qlens, dtype=torch.int32, device=dev)

    def cache():
        pc = ks._Paged(kd, vd, prefix, page, mp, 68, alloc_all=True)
        pc.k, pc.v = torch.nan_to_num(pc.k, nan=3.0), torch.nan_to_num(pc.v, nan=5.0)   # (finite: whole pools are compared)
        return pc

    pa, pb = cache(), cache()
    got = pkg.flash_attention_n_kvcache_tree(q, pa.k, pa.v, pa.lens, masks, block_table=pa.table, k_new=kn, v_new=vn, query_seqlens=qs, softmax_n_param=n,
                                             return_lse=True, rotary_cos=cos, rotary_sin=sin, rotary_interleaved=interleaved)
    dep = kt.depths(masks, ql).to(dev)
    base = torch.tensor(prefix, device=dev).view(B, 1)
    # len_b is clamped to the capacity: the query's base follows it, the key's position does not
    qbase = torch.tensor([min(p + x, page * mp) - x for p, x in zip(prefix, ql)], device=dev).view(B, 1)
    q_rot, k_rot = ks._rotate(q, qbase + dep, cos, sin, interleaved), ks._rotate(kn, base + dep, cos, sin, interleaved)
    want = pkg.flash_attention_n_kvcache_tree(q_rot, pb.k, pb.v, pb.lens, masks, block_table=pb.table, k_new=k_rot, v_new=vn, query_seqlens=qs,
                                              softmax_n_param=n, return_lse=True)
    assert torch.equal(ks._bits(pa.k), ks._bits(pb.k)) and torch.equal(ks._bits(pa.v), ks._bits(pb.v))
    assert torch.equal(ks._bits(got[0]), ks._bits(want[0])) and torch.equal(got[1], want[1])
    # ... and the pool is the old pool but for the rows base + i < capacity of the nodes i < qlen_b, which hold the eager rotation
    ref = cache()
    for b in range(B):
        for i in range(ql[b]):
            pos = prefix[b] + i
            if pos < page * mp:
                pid = int(ref.table[b, pos // page])
                ref.k[pid, pos % page], ref.v[pid, pos % page] = k_rot[b, :, i], vn[b, :, i]
    assert torch.equal(ks._bits(pa.k), ks._bits(ref.k)) and torch.equal(ks._bits(pa.v), ks._bits(ref.v))
    assert not torch.equal(ks._bits(k_rot), ks._bits(ks._rotate(kn, base + torch.arange(Sq, device=dev), cos, sin, interleaved)))   # depth != index
    # the self-only element: q decides through the sink's share, so a query rotated elsewhere shows
    off = pkg.flash_attention_n_kvcache_tree(ks._rotate(q, qbase + dep + 1, cos, sin, interleaved), pb.k, pb.v, pb.lens, masks, block_table=pb.table,
                                             query_seqlens=qs, softmax_n_param=n, k_new=k_rot, v_new=vn)
    assert not torch.equal(ks._bits(off[1]), ks._bits(got[0][1]))


# ---------------------------------------------------------------- 10: commit
def _commit_reference(k, v, table, page, base, accepted, alens):
    """through a temporary: all the sources are read before any destination is written"""
    k2, v2 = k.clone(), v.clone()
    for b, (bs, path, alen) in enumerate(zip(base, accepted, alens)):
        for kk in range(alen):
            src, dst = bs + path[kk], bs + kk
            ps, pd = (int(table[b, src // page]), int(table[b, dst // page])) if table is not None else (b, b)
            k2[pd, dst % page], v2[pd, dst % page] = k[ps, src % page], v[ps, src % page]
    return k2, v2


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("paged", [True, False], ids=["paged", "dense"])
def test_commit(pkg, dev, paged, dtype):
    """the whole pool bit for bit: the overlapping chain (row 2 is a source and a destination), the identity, an empty path, a path that
    ends at node Sq - 1; rows outside [base, base + alen) do not change"""
    Sq, Hkv, D, page, mp = 16, 2, 64, 64, 3
    base = [60, 5, 0, 128 - 3]
    accepted = [[0, 2, 3, 7], [0, 1, 2, 3], [0, 5, 9, 11], [0, 4, 9, 15]]
    alens = [4, 4, 0, 4]
    B = len(base)
    if paged:
        kd, vd = ks._rand((B, Hkv, page * mp, D), dtype, dev, 71), ks._rand((B, Hkv, page * mp, D), dtype, dev, 72, std=1.0)
        pc = ks._Paged(kd, vd, [b + Sq for b in base], page, mp, 73, alloc_all=True)
        k, v, table = torch.nan_to_num(pc.k, nan=3.0), torch.nan_to_num(pc.v, nan=5.0), pc.table
        tbl = table.cpu()
        assert sorted(tbl.flatten().tolist()) != tbl.flatten().tolist()        # shuffled
    else:
        k, v, table, tbl = ks._rand((B, page * mp, Hkv, D), dtype, dev, 71), ks._rand((B, page * mp, Hkv, D), dtype, dev, 72), None, None
    k_ref, v_ref = _commit_reference(k, v, tbl, page if paged else page * mp, base, accepted, alens)
    assert not torch.equal(k_ref, k)
    sl = torch.tensor(base, dtype=torch.int32, device=dev)
    pkg.flash_attention_n_kvcache_tree_commit(k, v, sl, torch.tensor(accepted, dtype=torch.int32, device=dev),
                                              torch.tensor(alens, dtype=torch.int32, device=dev), block_table=table)
    assert torch.equal(ks._bits(k), ks._bits(k_ref)) and torch.equal(ks._bits(v), ks._bits(v_ref))
    assert sl.tolist() == base
    # malformed paths: an index below k, beyond the nodes, a length beyond A - nothing outside [base, base + A) moves
    before_k, before_v = k.clone(), v.clone()
    bad = torch.tensor([[3, 0, 99, -4], [0, 1, 2, 3], [70, 70, 70, 70], [5, 4, 3, 2]], dtype=torch.int32, device=dev)
    pkg.flash_attention_n_kvcache_tree_commit(k, v, sl, bad, torch.tensor([99, -3, 4, 4], dtype=torch.int32, device=dev), block_table=table)
    changed = (ks._bits(k) != ks._bits(before_k)).any(-1).any(-1) | (ks._bits(v) != ks._bits(before_v)).any(-1).any(-1)   # [pages, rows]
    allowed = torch.zeros_like(changed)
    for b, bs in enumerate(base):
        for kk in range(4):
            pos = bs + kk
            allowed[int(tbl[b, pos // page]) if paged else b, pos % (page if paged else page * mp)] = True
    assert not (changed & ~allowed).any()


# ---------------------------------------------------------------- 11: end to end
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_end_to_end_verify_commit_advance(pkg, dev, dtype):
    """verify a random tree with rotary, commit a root-to-leaf path, advance the lengths: the cache is bit for bit the cache built by feeding
    the accepted tokens one at a time through flash_attention_n_kvcache_rope, the outputs at the accepted nodes match that route's"""
    B, H, Hkv, Sq, D, page, mp = 2, 8, 2, 16, 64, 64, 4
    prefix = [60, 131]
    gen = _gen(81)
    trees = [kt.random_tree(Sq, gen) for _ in range(B)]
    masks = kt.words_tensor([t[0] for t in trees], dev)
    paths = []
    for words, parents in trees:
        leaf = max(range(Sq), key=lambda i: (kt.depth(words[i], Sq), i))
        path = [t for t in range(Sq) if (words[leaf] >> t) & 1]
        assert path[0] == 0 and path[-1] == leaf and all(parents[b_] == a_ for a_, b_ in zip(path, path[1:]))
        paths.append(path)
    A = max(len(p) for p in paths)
    assert A >= 3
    acc = torch.tensor([p + [0] * (A - len(p)) for p in paths], dtype=torch.int32, device=dev)
    alens = torch.tensor([len(p) for p in paths], dtype=torch.int32, device=dev)
    n = ks._n_values((H,), dev, 82)
    q, kn, vn = ks._rand((B, H, Sq, D), dtype, dev, 83), ks._rand((B, Hkv, Sq, D), dtype, dev, 84), ks._rand((B, Hkv, Sq, D), dtype, dev, 85, std=1.0)
    cos, sin = ks._tables(page * mp, D, dev, torch.float32)
    kd, vd = ks._rand((B, Hkv, page * mp, D), dtype, dev, 86), ks._rand((B, Hkv, page * mp, D), dtype, dev, 87, std=1.0)
    pa, pb = (ks._Paged(kd, vd, prefix, page, mp, 88, alloc_all=True) for _ in range(2))
    out = pkg.flash_attention_n_kvcache_tree(q, pa.k, pa.v, pa.lens, masks, block_table=pa.table, k_new=kn, v_new=vn, softmax_n_param=n,
                                             rotary_cos=cos, rotary_sin=sin)
    pkg.flash_attention_n_kvcache_tree_commit(pa.k, pa.v, pa.lens, acc, alens, block_table=pa.table)
    # the sequential route: batch element b alone, one accepted token per call
    for b in range(B):
        sl = pb.lens[b:b + 1].clone()
        for kk, node in enumerate(paths[b]):
            o1 = pkg.flash_attention_n_kvcache_rope(q[b:b + 1, :, node:node + 1], pb.k, pb.v, sl, cos, sin, block_table=pb.table[b:b + 1],
                                                    k_new=kn[b:b + 1, :, node:node + 1], v_new=vn[b:b + 1, :, node:node + 1], softmax_n_param=n)
            ks._check(out[b:b + 1, :, node:node + 1], o1, dtype, f"end to end: sequence {b} node {node} (depth {kk})")
            sl += 1
    final = [p + len(path) for p, path in zip(prefix, paths)]
    for pool_a, pool_b in ((pa.k, pb.k), (pa.v, pb.v)):
        assert torch.equal(ks._bits(ks._gather(pool_a, pa.table, final, page)), ks._bits(ks._gather(pool_b, pb.table, final, page)))


# ---------------------------------------------------------------- 12, 13: graph replay, determinism
@pytest.mark.parametrize("route", ["decode", "prefill"])
def test_graph_replay_follows_the_device_operands(pkg, dev, route):
    dtype = torch.bfloat16
    B, H, Hkv, Sq, D, page, mp = (2, 8, 2, 13, 64, 64, 4) if route == "decode" else (2, 8, 1, 40, 64, 64, 4)
    q, kn, vn = ks._rand((B, H, Sq, D), dtype, dev, 91), ks._rand((B, Hkv, Sq, D), dtype, dev, 92), ks._rand((B, Hkv, Sq, D), dtype, dev, 93, std=1.0)
    kd, vd = ks._rand((B, Hkv, page * mp, D), dtype, dev, 94), ks._rand((B, Hkv, page * mp, D), dtype, dev, 95, std=1.0)
    cos, sin = ks._tables(page * mp, D, dev, torch.float32)
    pc = ks._Paged(kd, vd, [page * mp] * B, page, mp, 96)     # every row finite: the lengths move freely
    pool_k, pool_v = pc.k.clone(), pc.v.clone()
    sl = torch.tensor([60, 131], dtype=torch.int32, device=dev)
    masks = kt.words_tensor(_rows("tree", Sq, B, 97), dev)
    acc = torch.tensor([[0, 2, 5], [0, 1, 4]], dtype=torch.int32, device=dev)
    alens = torch.tensor([3, 2], dtype=torch.int32, device=dev)

    def step():
        o = pkg.flash_attention_n_kvcache_tree(q, pc.k, pc.v, sl, masks, block_table=pc.table, k_new=kn, v_new=vn, softmax_n_param=0.5, return_lse=True,
                                               rotary_cos=cos, rotary_sin=sin, window=100)
        pkg.flash_attention_n_kvcache_tree_commit(pc.k, pc.v, sl, acc, alens, block_table=pc.table)
        return o

    g, res = ks._capture(step)
    for new_sl, seed, new_acc, new_alens in (([60, 131], 97, [[0, 2, 5], [0, 1, 4]], [3, 2]), ([3, 190], 98, [[0, 1, 2], [0, 3, 9]], [1, 3])):
        sl.copy_(torch.tensor(new_sl, dtype=torch.int32))
        masks.copy_(kt.words_tensor(_rows("tree" if seed == 97 else "arbitrary", Sq, B, seed)))
        acc.copy_(torch.tensor(new_acc, dtype=torch.int32))
        alens.copy_(torch.tensor(new_alens, dtype=torch.int32))
        pc.k.copy_(pool_k), pc.v.copy_(pool_v)
        g.replay()
        got, got_k, got_v = [t.clone() for t in res], pc.k.clone(), pc.v.clone()
        pc.k.copy_(pool_k), pc.v.copy_(pool_v)
        want = step()
        assert torch.equal(ks._bits(got[0]), ks._bits(want[0])) and torch.equal(got[1], want[1])
        assert torch.equal(ks._bits(got_k), ks._bits(pc.k)) and torch.equal(ks._bits(got_v), ks._bits(pc.v))
        assert not torch.equal(ks._bits(got_k), ks._bits(pool_k))
    # ... and the eager result is the reference's (the first step's operands again)
    assert not torch.equal(ks._bits(res[0]), torch.zeros_like(ks._bits(res[0])))


@pytest.mark.parametrize("case", ["decode", "prefill", "split"])
def test_deterministic(pkg, dev, case):
    dtype = torch.bfloat16
    H, Hkv, Sq, prefix, mp = {"decode": (8, 2, 13, [60, 130], None), "prefill": (8, 1, 40, [70, 200], None), "split": (1, 1, 16, [3000], 64)}[case]
    if case == "split":
        assert _nsplit_decode(pkg, dtype, B=1, H=1, Hkv=1, Sq=16, D=64, page=64, max_pages=64) > 1
    B = len(prefix)
    q, pc = ks._case(dev, B, H, Hkv, Sq, 64, dtype, 64, [p + Sq for p in prefix], 99, mp)
    masks = kt.words_tensor(_rows("arbitrary", Sq, B, 5), dev)
    runs = [pkg.flash_attention_n_kvcache_tree(q, pc.k, pc.v, pc.lens, masks, block_table=pc.table, softmax_n_param=0.25, return_lse=True) for _ in range(2)]
    assert torch.equal(ks._bits(runs[0][0]), ks._bits(runs[1][0])) and torch.equal(runs[0][1], runs[1][1])
    assert math.isfinite(runs[0][0].float().abs().sum().item())
