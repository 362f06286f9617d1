"""flash_attention_n_mla_index on the GPU against plain fp64 torch: logit = sum_h w_h relu(q_h . k_j) by einsum, the list = stable descending
sort of logit[:L], cut at topk, sorted ascending, -1 behind it. One set-up throughout: a paged cache of 64-row pages behind a scrambled
block table, capacity 6144, B = 3 with unequal lengths, every row at or beyond an element's length and every page no table names NaN
(kv_support._Paged) - so every case is also the poison case: a stale row or an unnamed page that is read shows as NaN or as a wrong entry."""
import functools

import pytest
import torch

from kv_support import _bits, _capture, _check, _check_lse, _Paged, _rand

pytestmark = pytest.mark.gpu
D, PAGE, PAGES, B = 128, 64, 96, 3
CAP = PAGE * PAGES
DTYPES = [torch.float16, torch.bfloat16]
W_VALUES = (-2.0, -1.0, -0.5, 0.5, 1.0, 2.0)


def _ints(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def _data(dtype, Hi, Sq, exact, seed=0, dev="cuda"):
    """q [B, Hi, Sq, 128], w [B, Hi, Sq] - the model's [B, Sq, Hi] transposed, a strided view -, dense keys [B, 1, CAP, 128], and in fp64
    the logits [B, Sq, CAP] and sum_h |w_h| sum_d |q_hd k_d|. exact: q, k from {-2 .. 2} and w from {+-0.5, +-1, +-2} - every partial sum
    is a multiple of 0.5 below 2^17, so fp32 is exact in any order, and the key at position j is row (j // 2) % 40 of 40 drawn rows, so that
    every logit has equals next to it and far away and every cut of the lengths below runs through a tie; otherwise seeded normal values,
    every row of its own."""
    if exact:
        q = _ints((B, Hi, Sq, D), -2, 2, seed + 1).to(dtype).to(dev)
        k = _ints((B, 1, 40, D), -2, 2, seed + 2)[:, :, (torch.arange(CAP) // 2) % 40].to(dtype).to(dev)
        w = torch.tensor(W_VALUES)[_ints((B, Sq, Hi), 0, 5, seed + 3)].to(dev).transpose(1, 2)
    else:
        q, k = _rand((B, Hi, Sq, D), dtype, dev, seed + 1, std=1.0), _rand((B, 1, CAP, D), dtype, dev, seed + 2, std=1.0)
        w = _rand((B, Sq, Hi), torch.float32, dev, seed + 3, std=1.0).transpose(1, 2)
    qd, kd, wd = q.double(), k[:, 0].double(), w.double()[..., None]
    logits = (wd * torch.einsum("bhqd,bsd->bhqs", qd, kd).relu()).sum(1)
    mag = (wd.abs() * torch.einsum("bhqd,bsd->bhqs", qd.abs(), kd.abs())).sum(1)
    return q, w, k, logits, mag


def _visible(lens, Sq, causal):
    """L of every row (b, i): len_b - (Sq - 1 - i) when causal, len_b otherwise"""
    return [[ln - (Sq - 1 - i) if causal else ln for i in range(Sq)] for ln in lens]


def _select(logits, Ls, topk):
    """the reference list [B, Sq, topk] int32 of logits [B, Sq, >= L], and whether some row has a tie at its cut"""
    out, tie = torch.full(tuple(logits.shape[:2]) + (topk,), -1, dtype=torch.int32, device=logits.device), False
    for b, row in enumerate(Ls):
        for i, L in enumerate(row):
            if L > 0:
                v, order = torch.sort(logits[b, i, :L], descending=True, stable=True)
                out[b, i, :min(L, topk)] = order[:topk].sort().values.int()
                tie |= L > topk and bool(v[topk - 1] == v[topk])
    return out, tie


def _hidden_is_neg_inf(lg, Ls):
    return all((lg[b, i, max(L, 0):] == float("-inf")).all() for b, row in enumerate(Ls) for i, L in enumerate(row))


def _call(pkg, q, w, pc, topk, causal, **kw):
    return pkg.flash_attention_n_mla_index(q, w, pc.k, pc.lens, topk, block_table=pc.table, is_causal=causal, return_logits=True, **kw)


@pytest.mark.parametrize("causal", [True, False], ids=["c", "nc"])
@pytest.mark.parametrize("Sq", [1, 2])
@pytest.mark.parametrize("Hi", [32, 64])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_exact_parity(pkg, dtype, Hi, Sq, causal):
    """integer-valued inputs: the list and the logits are exact, at topk = 64 and at topk = 2048 (one item runs both: they share the
    queries, the keys and the reference). The lengths walk through the tile seam, the shortcut / select seam, a ragged last tile,
    several select chunks and a full cache: over the 16 items every value of both lists occurs for either topk, and the third element is
    always long enough to be selected from."""
    c = ((DTYPES.index(dtype) * 2 + Hi // 64) * 2 + Sq - 1) * 2 + causal
    q, w, k, ref, _ = _data(dtype, Hi, Sq, True)
    for topk in (64, 2048):
        short, long_ = [0, 1, 63, 64, 65, topk - 1, topk], [topk + 1, 2373, 5000, CAP]
        lens = [short[2 * c % 7], short[(2 * c + 1) % 7], long_[c % 4]]
        pc, Ls = _Paged(k, k, lens, PAGE, PAGES, c), _visible(lens, Sq, causal)
        idx, lg = _call(pkg, q, w, pc, topk, causal)
        want, tie = _select(ref, Ls, topk)
        assert tie, f"topk {topk}: no row has a tie at its cut: the tie rule is not exercised"
        assert idx.dtype == torch.int32 and idx.is_contiguous() and torch.equal(idx, want), (topk, lens)
        assert all(torch.equal(lg[b, i, :max(L, 0)].double(), ref[b, i, :max(L, 0)]) for b, row in enumerate(Ls) for i, L in enumerate(row)), (topk, lens)
        assert _hidden_is_neg_inf(lg, Ls), (topk, lens)


@pytest.mark.parametrize("Hi", [32, 64])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_real_valued_parity(pkg, dtype, Hi):
    """|logit - ref64| <= gamma sum_h |w_h| sum_d |q_hd k_d|, gamma = (128 + Hi + 2) 2^-23: products of 16-bit numbers are exact in fp32 and
    each of the at most 128 + Hi + 2 fp32 operations loses at most one ulp. The list is the reference rule on the call's own logits."""
    Sq, topk, lens = 2, 2048, [65, 2373, CAP]
    q, w, k, ref, mag = _data(dtype, Hi, Sq, False)
    pc, Ls = _Paged(k, k, lens, PAGE, PAGES, 7), _visible(lens, Sq, True)
    idx, lg = _call(pkg, q, w, pc, topk, True)
    gamma = (128 + Hi + 2) * 2.0 ** -23
    for b, row in enumerate(Ls):
        for i, L in enumerate(row):
            err, lim = (lg[b, i, :L].double() - ref[b, i, :L]).abs(), gamma * mag[b, i, :L]
            print(f"{dtype} Hi={Hi} row ({b}, {i}): max err / bound {float((err / lim).max()):.3f}")
            assert (err <= lim).all()
    assert _hidden_is_neg_inf(lg, Ls) and torch.equal(idx, _select(lg, Ls, topk)[0])


@pytest.mark.parametrize("Sq", [1, 2])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_k_new(pkg, dtype, Sq):
    """the call with k_new = the call on a cache into which torch wrote the rows, lengths advanced; the cache bytes agree afterwards. One
    element sits at capacity - 1 and one at capacity: rows are dropped for either Sq."""
    lens = [5, CAP - 1, CAP]
    q, w, k, _, _ = _data(dtype, 64, Sq, True)
    pc = _Paged(k, k, lens, PAGE, PAGES, 9, alloc_all=True)
    k_new = _ints((B, Sq, 1, D), -2, 2, 10).to(dtype).to(q.device)
    pool, want = pc.k.clone(), pc.k.clone()
    for b, ln in enumerate(lens):
        for i in range(min(Sq, CAP - ln)):
            want[int(pc.table[b, (ln + i) // PAGE]), (ln + i) % PAGE] = k_new[b, i]
    got = pkg.flash_attention_n_mla_index(q, w, pool, pc.lens, 64, block_table=pc.table, k_new=k_new, return_logits=True)
    assert torch.equal(_bits(pool), _bits(want))
    ref = pkg.flash_attention_n_mla_index(q, w, want, pc.lens + Sq, 64, block_table=pc.table, return_logits=True)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]) and (got[0][0, -1, :5 + Sq] == torch.arange(5 + Sq, device=q.device)).all()


def test_one_graph(pkg):
    """one capture, replayed over four sets of lengths with changed cache contents (the rows rolled along the positions, and the reference
    with them): every replay is the exact reference"""
    dtype, Hi, Sq, topk = torch.bfloat16, 64, 2, 2048
    q, w, k, ref, _ = _data(dtype, Hi, Sq, True)
    pc = _Paged(k, k, [CAP] * B, PAGE, PAGES, 11, alloc_all=True)
    graph, res = _capture(lambda: _call(pkg, q, w, pc, topk, True))
    for step, lens in enumerate(([0, 0, 0], [CAP, CAP, CAP], [2049, 1, 5000], [64, 4097, 2048])):
        k2, ref2 = k.roll(577 * step, 2), ref.roll(577 * step, 2)
        new = _Paged(k2, k2, lens, PAGE, PAGES, 11, alloc_all=True)   # (the same seed and pages: the same table)
        assert torch.equal(new.table, pc.table)
        pc.k.copy_(new.k)
        pc.lens.copy_(new.lens)
        graph.replay()
        Ls = _visible(lens, Sq, True)
        assert torch.equal(res[0], _select(ref2, Ls, topk)[0]) and _hidden_is_neg_inf(res[1], Ls), lens
        assert all(torch.equal(res[1][b, i, :max(L, 0)].double(), ref2[b, i, :max(L, 0)]) for b, row in enumerate(Ls) for i, L in enumerate(row)), lens


def test_end_to_end_with_the_sparse_decode(pkg):
    """topk >= L: the list is every visible position, and flash_attention_n_mla_sparse behind it is flash_attention_n_mla"""
    from mla_support import SCALE, _cache
    dtype, Sq, lens = torch.bfloat16, 2, (0, 1, 65, 1100)
    latent, _ = _cache(dtype, 64, lens, False, 13)
    dev, nb = latent.k.device, len(lens)
    keys = _rand((nb, 1, CAP, D), dtype, dev, 14)
    pc = _Paged(keys, keys, list(lens), PAGE, PAGES, 15)
    qi, wi = _rand((nb, 32, Sq, D), dtype, dev, 16), _rand((nb, 32, Sq), torch.float32, dev, 17)
    idx = pkg.flash_attention_n_mla_index(qi, wi, pc.k, pc.lens, 2048, block_table=pc.table)
    assert torch.equal(idx, _select(torch.zeros(nb, Sq, CAP, device=dev), _visible(lens, Sq, True), 2048)[0])
    q = _rand((nb, 16, Sq, 576), dtype, dev, 18)
    want = pkg.flash_attention_n_mla(q, latent.k, latent.lens, SCALE, block_table=latent.table, return_lse=True)
    got = pkg.flash_attention_n_mla_sparse(q, latent.k, idx, latent.lens, SCALE, block_table=latent.table, return_lse=True)
    _check(got[0], want[0], dtype, "index -> sparse out")
    _check_lse(got[1], want[1], "index -> sparse lse")
