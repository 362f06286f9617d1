"""flash_attention_n_kvcache_shared_prefix on the GPU: decode behind a shared prefix equals flash_attention_n_kvcache on the virtual cache
(tests/kv_prefix.py) - parity with two witnesses, rows of one sequence in two row blocks, P between the limits of one sequence's rows,
the memory contract, every key once and the sink once (kv_witness A), one key decides (kv_witness B), the base call on truly shared
tables, the append, one captured graph for every prefix, and the refusals. Page 64 unless said."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_prefix as sp      # noqa: E402
import kv_support as ks     # noqa: E402
import kv_witness as kw     # noqa: E402

pytestmark = pytest.mark.gpu
PAGE = 64
PREFIXES = [0, 1, 63, 64, 65, PAGE + 1, 2 * PAGE + 37]
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
HEADS = [(8, 2), (4, 4), (8, 1)]
PARITY = [(D, dt, hh, Sq) for D in (64, 128) for dt in ("fp16", "bf16") for hh in HEADS for Sq in (1, 4)]


def _n(kind, B, H, dev, seed):
    return {0: 1.0, 1: 0.0, 2: ks._n_values((B, H), dev, seed)}[kind % 3]


@pytest.mark.parametrize("i", range(len(PARITY)))
def test_parity_on_the_virtual_cache(pkg, dev, i):
    """an empty suffix (len_b = P), a sequence shorter than the prefix, an empty sequence; P walks PREFIXES over the parametrisation"""
    D, dt, (H, Hkv), Sq = PARITY[i]
    dtype, P = DTYPES[dt], PREFIXES[i % len(PREFIXES)]
    lens = [3 * PAGE + 1, P, 37, 0, 2 * PAGE]
    q, kd, vd = sp.data(dev, 5, H, Hkv, Sq, D, dtype, PAGE, 5, 100 + i)
    sh = sp.Shared(kd, vd, lens, P, PAGE, 5, 7 + i, prefix_pages=3)
    n = _n(i, 5, H, dev, 50 + i)
    for causal in (True, False):
        out, lse = sp.shared_call(pkg, sh, q, n, causal)
        sp.check(pkg, sh, out, lse, q, n, causal, dtype, f"D={D} {dt} H={H}/{Hkv} Sq={Sq} P={P} causal={causal}")


@pytest.mark.parametrize("plen,P", [(-5, 0), (10000, 2 * PAGE), (-2 ** 31, 0), (2 ** 31 - 1, 2 * PAGE)])
def test_prefix_len_is_clamped(pkg, dev, plen, P):
    """prefix_len below 0 and beyond max_prefix_pages * page: the kernels clamp it"""
    lens = [3 * PAGE + 1, P, 37, 0, 2 * PAGE]
    q, kd, vd = sp.data(dev, 5, 8, 2, 4, 64, torch.bfloat16, PAGE, 5, 31)
    sh = sp.Shared(kd, vd, lens, P, PAGE, 5, 3, prefix_pages=2)
    n = ks._n_values((5, 8), dev, 9)
    out, lse = sp.shared_call(pkg, sh, q, n, True, prefix_len=torch.tensor([plen], dtype=torch.int32, device=dev))
    sp.check(pkg, sh, out, lse, q, n, True, torch.bfloat16, f"prefix_len={plen}")


@pytest.mark.parametrize("D,dt", [(64, "bf16"), (128, "fp16")])
def test_rows_of_one_sequence_in_two_row_blocks(pkg, dev, D, dt):
    """R = 15, B = 10: the rows 120 .. 134 of sequence 8 sit in two blocks and the second block is mostly idle"""
    dtype = DTYPES[dt]
    lens = [130, 100, 37, 200, 99, 101, 64, 1, 180, 150]
    q, kd, vd = sp.data(dev, 10, 6, 2, 5, D, dtype, PAGE, 4, 61)
    sh = sp.Shared(kd, vd, lens, 100, PAGE, 4, 5, prefix_pages=2)
    n = ks._n_values((10, 6), dev, 8)
    for causal in (True, False):
        out, lse = sp.shared_call(pkg, sh, q, n, causal)
        sp.check(pkg, sh, out, lse, q, n, causal, dtype, f"straddle D={D} {dt} causal={causal}")


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("D", [64, 128])
def test_prefix_ends_between_the_limits_of_one_sequences_rows(pkg, dev, D, causal):
    """Sq = 4, len_b = 70, P = 68: the causal limits 66 .. 69 lie on either side of P"""
    q, kd, vd = sp.data(dev, 2, 8, 2, 4, D, torch.float16, PAGE, 3, 71)
    sh = sp.Shared(kd, vd, [70, 70], 68, PAGE, 3, 11)
    for n in (1.0, 0.0):
        out, lse = sp.shared_call(pkg, sh, q, n, causal)
        sp.check(pkg, sh, out, lse, q, n, causal, torch.float16, f"P=68 len=70 D={D} causal={causal} n={n}")


@pytest.mark.parametrize("D,dt", [(64, "fp16"), (128, "bf16")])
def test_memory_contract(pkg, dev, D, dt):
    """what the contract lets hold anything holds NaN or points at the poison page; the output is finite and passes the gates"""
    dtype, P = DTYPES[dt], 2 * PAGE + 37
    lens = [3 * PAGE + 1, P, 37, 0, 2 * PAGE, 4 * PAGE]
    q, kd, vd = sp.data(dev, 6, 8, 2, 4, D, dtype, PAGE, 5, 81)
    sh = sp.Shared(kd, vd, lens, P, PAGE, 5, 13, prefix_pages=4)
    tab, ptab = sh.table.cpu(), sh.prefix_table.cpu()
    assert torch.isnan(sh.k[sh.poison]).all() and torch.isnan(sh.v[sh.poison]).all()
    assert (tab[:, :P // PAGE] == sh.poison).all()                                   # own slots wholly below P
    assert (ptab[-(-P // PAGE):] == sh.poison).all() and len(ptab) == 4              # prefix_table beyond ceil(P / page)
    last = int(ptab[P // PAGE])
    assert torch.isnan(sh.k[last, P % PAGE:]).all() and torch.isfinite(sh.k[last, :P % PAGE]).all()   # prefix-page rows at or beyond P
    for b in (0, 5):                                                                 # own rows below P in the partially shared page
        own = int(tab[b, P // PAGE])
        assert own != sh.poison and torch.isnan(sh.v[own, :P % PAGE]).all() and torch.isfinite(sh.v[own, P % PAGE]).all()
    own = int(tab[0, 3])
    assert torch.isnan(sh.k[own, 1:]).all()                                          # rows at or beyond len_b
    n = ks._n_values((6, 8), dev, 4)
    for causal in (True, False):
        out, lse = sp.shared_call(pkg, sh, q, n, causal)
        assert torch.isfinite(out).all() and not torch.isnan(lse).any()
        sp.check(pkg, sh, out, lse, q, n, causal, dtype, f"contract D={D} {dt} causal={causal}")


@pytest.mark.parametrize("nkind", ["zero", "one", "tensor"])
@pytest.mark.parametrize("P", [63, 64, 65])
@pytest.mark.parametrize("D,dt,Sq", [(64, "bf16", 1), (128, "fp16", 3)])
def test_every_key_once_and_the_sink_once(pkg, dev, D, dt, Sq, P, nkind):
    """kv_witness A: query 0 and indicator V - exp(lse) = n + visible keys, out Z counts the keys of a class. len_b on either side of P"""
    dtype = DTYPES[dt]
    case = sp.witness_case(8, 2, D, Sq, [40, 62, 63, 64, 65, 66, 130, 200, 0])
    inp = kw.inputs_a(case, dtype, dev, 5 + P)
    if nkind == "tensor":
        inp["n"] = ks._n_values((case.B, case.H), dev, 17)
        assert (inp["n"] == 0).any() and (inp["n"] > 0).any()
    else:
        inp["n"] = torch.tensor(0.0 if nkind == "zero" else 1.0, device=dev)
    got, seen = sp.shared_witness_run(pkg, case, inp, P)
    refs = kw.reference(case, seen)
    kw.condition_a(refs, dtype)
    ratios = [kw.gate_a(o, lse, r) for (o, lse), r in zip(got, refs)]
    rz, ro = max(r[0] for r in ratios), max(r[1] for r in ratios)
    print(f"A P={P} n={nkind}: exp(lse) at {rz:.3g} of 1e-5 Z, out Z at {ro:.3g} of 0.25")
    assert rz <= 1, f"exp(lse) is {rz:.3g}x (1e-5 Z_ref) from n + the number of visible keys, per sequence {[r[0] for r in ratios]}"
    assert ro <= 1, f"out Z_ref is {ro:.3g}x 0.25 from the class counts, per sequence {[r[1] for r in ratios]}"


@pytest.mark.parametrize("form", kw.B_FORMS)
@pytest.mark.parametrize("D,dt,Sq,P", [(64, "fp16", 1, 100), (128, "bf16", 3, 64), (64, "bf16", 2, 65)])
def test_one_key_decides(pkg, dev, D, dt, Sq, P, form):
    """kv_witness B, scale 32: ascending - the last visible key decides, below P where len_b <= P and at or above P elsewhere; descending -
    key 0, in the prefix, against a suffix partial; sink - the sink decides the rows with n > 0. A partial merged with the wrong weight
    gives another key's V row."""
    dtype = DTYPES[dt]
    case = sp.witness_case(8, 2, D, Sq, [40, P - 1, P, P + 1, P + 2, 130, 200, 3, 0])
    inp = kw.inputs_b(case, form, dtype, dev, 23)
    got, seen = sp.shared_witness_run(pkg, case, inp, P)
    refs = kw.reference(case, seen)
    ratios, kinds = [], set()
    for b, ((o, lse), r) in enumerate(zip(got, refs)):
        kind, want = kw.expect_b(r, kw.sequence(case, seen, b)[2][:, :case.total[b]], case.H // case.Hkv)
        kinds |= set(kind.unique().tolist())
        ratios.append(kw.gate_b(o, kind, want, dtype))
        ks._check_lse(lse, r["lse"].float(), f"B {form} sequence {b} lse")
    print(f"B P={P} {form} {dt}: out at {max(ratios):.3g} of its gate; row kinds {sorted(kinds)}")
    assert max(ratios) <= 1, f"out is {max(ratios):.3g}x the gate from the deciding key's V row, per sequence {ratios}"
    assert 1 in kinds or form == "sink"


@pytest.mark.parametrize("D,dt,Sq", [(64, "bf16", 1), (128, "fp16", 4)])
def test_against_the_base_call(pkg, dev, D, dt, Sq):
    """tables that truly share the prefix pages: the base call walks the same virtual cache. prefix_len = 0: the same split rule, the
    same walk, a skipped neutral partial - bit for bit the base call"""
    dtype, P = DTYPES[dt], 2 * PAGE
    lens = [3 * PAGE + 1, P, 37, 0, 2 * PAGE + 5, 6 * PAGE]
    q, kd, vd = sp.data(dev, 6, 8, 2, Sq, D, dtype, PAGE, 7, 91)
    sh = sp.Shared(kd, vd, lens, P, PAGE, 7, 17, share=True)
    n = ks._n_values((6, 8), dev, 6)
    for causal in (True, False):
        base, base_lse = pkg.flash_attention_n_kvcache(q, sh.k, sh.v, sh.lens, block_table=sh.table, softmax_n_param=n, is_causal=causal, return_lse=True)
        out, lse = sp.shared_call(pkg, sh, q, n, causal)
        ks._check(out, base.float(), dtype, f"vs base D={D} causal={causal} out")
        ks._check_lse(lse, base_lse, f"vs base D={D} causal={causal} lse")
        print(f"max |shared - base| = {(out.float() - base.float()).abs().max().item():.3e}")
        out0, lse0 = sp.shared_call(pkg, sh, q, n, causal, prefix_len=torch.zeros(1, dtype=torch.int32, device=dev))
        assert torch.equal(out0, base) and torch.equal(lse0, base_lse), "prefix_len = 0 is not the base call bit for bit"


@pytest.mark.parametrize("D,dt", [(64, "fp16"), (128, "bf16")])
def test_append(pkg, dev, D, dt):
    """k_new / v_new go to the sequence's own pages at cache_seqlens[b] + i: where that is at or beyond P they are attended to, where it
    is below P (rows 90 .. 93 under P = 100) they are never read"""
    dtype, P, Sq, B = DTYPES[dt], 100, 4, 4
    old = [110, 90, 98, 100]
    q, kd, vd = sp.data(dev, B, 8, 2, Sq, D, dtype, PAGE, 4, 41)
    sh = sp.Shared(kd, vd, old, P, PAGE, 4, 19, alloc_all=True)
    kn = torch.stack([sh.kd[b, :, old[b]:old[b] + Sq] for b in range(B)])
    vn = torch.stack([sh.vd[b, :, old[b]:old[b] + Sq] for b in range(B)])
    n = ks._n_values((B, 8), dev, 2)
    out, lse = sp.shared_call(pkg, sh, q, n, True, k_new=kn, v_new=vn)
    new = [ln + Sq for ln in old]
    kg, vg = sh.gather(new)
    assert torch.equal(kg, ks._visible_dense(sh.kd, new)[:, :, :kg.shape[2]]) and torch.equal(vg, ks._visible_dense(sh.vd, new)[:, :, :vg.shape[2]])
    sp.check(pkg, sh, out, lse, q, n, True, dtype, f"append D={D} {dt}", lens=new)


def test_one_graph_serves_every_prefix(pkg, dev):
    """captured once; prefix_len, prefix_table, cache_seqlens, block_table (and the cache) change in place: the replay is the eager call"""
    dtype, B, H, Hkv, Sq, D = torch.bfloat16, 5, 8, 2, 2, 64
    builds = []
    for seed, P, lens in ((1, 2 * PAGE + 37, [200, 165, 37, 0, 256]), (2, 65, [66, 3, 190, 64, 65]), (3, 0, [1, 0, 256, 64, 100])):
        q, kd, vd = sp.data(dev, B, H, Hkv, Sq, D, dtype, PAGE, 4, 10 * seed)
        builds.append((q, sp.Shared(kd, vd, lens, P, PAGE, 4, seed, prefix_pages=3, alloc_all=True)))
    n = ks._n_values((B, H), dev, 12)
    names = ("k", "v", "lens", "table", "prefix_table", "plen")
    q0, sh0 = builds[0]
    static = {a: getattr(sh0, a).clone() for a in names}
    qs = q0.clone()

    def run():
        return pkg.flash_attention_n_kvcache_shared_prefix(qs, static["k"], static["v"], static["lens"], static["table"], static["prefix_table"],
                                                           static["plen"], softmax_n_param=n, return_lse=True)
    g, (out, lse) = ks._capture(run)
    for q, sh in builds[::-1]:
        qs.copy_(q)
        for a in names:
            static[a].copy_(getattr(sh, a))
        g.replay()
        torch.cuda.synchronize()
        want, want_lse = sp.shared_call(pkg, sh, q, n, True)
        assert torch.equal(out, want) and torch.equal(lse, want_lse), f"replay differs from the eager call at P = {sh.P}"
        sp.check(pkg, sh, out, lse, q, n, True, dtype, f"graph P={sh.P}")


def test_refusals_name_their_reason(pkg, dev):
    fa = pkg.flash_attention_n_kvcache_shared_prefix
    q, kd, vd = sp.data(dev, 2, 8, 2, 1, 64, torch.float16, PAGE, 3, 5)
    sh = sp.Shared(kd, vd, [70, 100], 64, PAGE, 3, 1)
    args = (q, sh.k, sh.v, sh.lens, sh.table, sh.prefix_table, sh.plen)
    with pytest.raises(ValueError, match="a dense cache .block_table=None. is not supported"):
        fa(q, sh.k, sh.v, sh.lens, None, sh.prefix_table, sh.plen)
    with pytest.raises(TypeError, match="a float8 cache is not supported"):
        fa(q, sh.k.to(torch.float8_e4m3fn), sh.v.to(torch.float8_e4m3fn), *args[3:])
    for D in (32, 256):
        with pytest.raises(ValueError, match=r"head dim %d is not supported behind a shared prefix \(supported: \(64, 128\)" % D):
            fa(q[..., :1].expand(-1, -1, -1, D), *args[1:])
    with pytest.raises(ValueError, match="rows exceed the 128 of one pass"):
        fa(torch.zeros(2, 8, 33, 64, dtype=torch.float16, device=dev), *args[1:])
    for bad in (sh.prefix_table.long(), sh.prefix_table.view(1, -1), sh.prefix_table[:0], sh.prefix_table[::2], [1, 2]):
        with pytest.raises(ValueError, match="prefix_table must be a contiguous int32 tensor of shape .max_prefix_pages."):
            fa(*args[:5], bad, sh.plen)
    for bad in (sh.plen.long(), torch.zeros(2, dtype=torch.int32, device=dev), 64, sh.plen.float()):
        with pytest.raises(ValueError, match="prefix_len must be an int32 tensor of one element"):
            fa(*args[:6], bad)
    with pytest.raises(RuntimeError, match="prefix_table is on cpu"):
        fa(*args[:5], sh.prefix_table.cpu(), sh.plen)
    with pytest.raises(RuntimeError, match="prefix_len is on cpu"):
        fa(*args[:6], sh.plen.cpu())
    with pytest.raises(RuntimeError, match="forward only"):
        fa(q.clone().requires_grad_(), *args[1:])
    out = fa(*args)   # what is refused above is not this call's shape
    assert out.shape == q.shape and torch.isfinite(out).all()
