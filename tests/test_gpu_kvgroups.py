"""flash_attention_n_kvcache_prefix_groups on the GPU: decode behind several shared prefixes in one call equals flash_attention_n_kvcache
on the virtual cache (tests/kv_prefix.py) - parity with two witnesses over interleaved groups, groups without members, a group whose rows
fill more than one item; bit equality with the shared-prefix call (G = 1) and with the base call (nobody grouped); prefix_lens clamped per
group; the memory contract; every key once and the sink once (kv_witness A), one key decides (kv_witness B); the schedule table against
its integer model; the append; one captured graph for every assignment; and the refusals. Page 64, at most 512 keys, B at most 40 - but
for the table alone, at B = 300."""
import os
import random
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_prefix as kg      # noqa: E402
import kv_support as ks     # noqa: E402
import kv_witness as kw     # noqa: E402

pytestmark = pytest.mark.gpu
PAGE = 64
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
MIXED = [1, 0, 2, 0, -1, 1, 0]                 # interleaved: the order table is not the identity
MIXED_PLENS = (130, 64, 200)
MIXED_LENS = [300, 250, 210, 64, 100, 37, 131]   # b = 3 (group 0, P = 130) and b = 5 (group 1, P = 64) are shorter than their prefixes
# the assignments of the parity tests, for the schedule-table test too: name -> (H, Hkv, Sq, group, G)
SPARSE = [15, 3, -1, 3, 15]
STRADDLE = [0, 1, 0, 0, 1, 0, 0, 0, -1, 0, 1, 0, 0, 0]   # group 0: 10 sequences of R = 15 rows, group 1: 3
BIG = [0] * 12 + [1, -1] + [0] * 10 + [1, 1, 5] + [0] * 11 + [1, -1]   # B = 40: 33 in group 0, 4 in group 1
ASSIGNMENTS = {"mixed": (8, 2, 3, MIXED, 3), "sparse": (8, 2, 1, SPARSE, 16), "straddle": (6, 2, 5, STRADDLE, 2), "big": (8, 2, 1, BIG, 2)}


def _n(kind, B, H, dev, seed):
    return {0: 1.0, 1: 0.0, 2: ks._n_values((B, H), dev, seed)}[kind % 3]


def _both(pkg, gr, q, n, dtype, what):
    for causal in (True, False):
        out, lse = kg.groups_call(pkg, gr, q, n, causal)
        kg.check(pkg, gr, out, lse, q, n, causal, dtype, f"{what} causal={causal}")


PARITY = [(D, dt, Sq) for D in (64, 128) for dt in ("fp16", "bf16") for Sq in (1, 3)]


@pytest.mark.parametrize("i", range(len(PARITY)))
def test_parity_interleaved_groups(pkg, dev, i):
    """B = 7, groups [1, 0, 2, 0, -1, 1, 0] behind prefixes of 130, 64 and 200 keys; causal and not"""
    D, dt, Sq = PARITY[i]
    dtype = DTYPES[dt]
    q, kd, vd = kg.data(dev, 7, 8, 2, Sq, D, dtype, PAGE, 5, 200 + i)
    gr = kg.Groups(kd, vd, MIXED_LENS, MIXED, MIXED_PLENS, PAGE, 5, 7 + i, prefix_pages=4)
    assert gr.Pb == [64, 130, 200, 130, 0, 64, 130]
    _both(pkg, gr, q, _n(i, 7, 8, dev, 50 + i), dtype, f"mixed D={D} {dt} Sq={Sq}")


@pytest.mark.parametrize("D,dt", [(64, "bf16"), (128, "fp16")])
def test_parity_groups_without_members(pkg, dev, D, dt):
    """G = 16, members in groups 3 and 15 only: fourteen table rows that no item names"""
    dtype = DTYPES[dt]
    plens = [100] * 16
    plens[3], plens[15] = 70, 129
    q, kd, vd = kg.data(dev, 5, 8, 2, 1, D, dtype, PAGE, 4, 230)
    gr = kg.Groups(kd, vd, [200, 71, 90, 64, 256], SPARSE, plens, PAGE, 4, 3, prefix_pages=3)
    assert (gr.prefix_tables[[g for g in range(16) if g not in (3, 15)]] == gr.poison).all()
    _both(pkg, gr, q, ks._n_values((5, 8), dev, 3), dtype, f"sparse D={D} {dt}")


@pytest.mark.parametrize("D,dt", [(64, "fp16"), (128, "bf16")])
def test_parity_a_group_in_two_items(pkg, dev, D, dt):
    """(H, Hkv, Sq) = (6, 2, 5): the 10 sequences of group 0 have 150 rows in two items, the rows 120 .. 134 of its ninth member straddle
    them; group 1 (3 sequences) starts at row 150, in an item of its own"""
    dtype = DTYPES[dt]
    lens = [130, 100, 37, 200, 99, 101, 64, 5, 180, 150, 256, 70, 129, 128]
    q, kd, vd = kg.data(dev, 14, 6, 2, 5, D, dtype, PAGE, 4, 261)
    gr = kg.Groups(kd, vd, lens, STRADDLE, (100, 65), PAGE, 4, 5, prefix_pages=2)
    order, slot, items, _, _ = kg.model(STRADDLE, 2, 15)
    assert items == [(0, 0, 150), (0, 128, 150), (1, 150, 195)] and slot[order[8]] * 15 < 128 < slot[order[8]] * 15 + 15
    _both(pkg, gr, q, ks._n_values((14, 6), dev, 8), dtype, f"straddle D={D} {dt}")


@pytest.mark.parametrize("D,dt", [(64, "bf16"), (128, "fp16")])
def test_parity_a_group_of_33(pkg, dev, D, dt):
    """B = 40, R = 4: the 132 rows of group 0 are one full item and four rows of a second"""
    dtype = DTYPES[dt]
    rnd = random.Random(5)
    lens = [rnd.choice([0, 1, 63, 64, 65, 100, 128, 129, 191, 192]) for _ in range(40)]
    q, kd, vd = kg.data(dev, 40, 8, 2, 1, D, dtype, PAGE, 3, 290)
    gr = kg.Groups(kd, vd, lens, BIG, (129, 64), PAGE, 3, 9, prefix_pages=3)
    assert kg.model(BIG, 2, 4)[2] == [(0, 0, 132), (0, 128, 132), (1, 132, 148)]
    _both(pkg, gr, q, ks._n_values((40, 8), dev, 4), dtype, f"33 of 40 D={D} {dt}")


# ---------------------------------------------------------------- against the calls that exist, bit for bit
@pytest.mark.parametrize("D,dt,Sq", [(64, "bf16", 1), (128, "fp16", 3)])
def test_one_group_is_the_shared_prefix_call(pkg, dev, D, dt, Sq):
    dtype, P = DTYPES[dt], 2 * PAGE + 37
    lens = [3 * PAGE + 1, P, 37, 0, 2 * PAGE, 5 * PAGE]
    q, kd, vd = kg.data(dev, 6, 8, 2, Sq, D, dtype, PAGE, 5, 301)
    sh = kg.Shared(kd, vd, lens, P, PAGE, 5, 7, prefix_pages=3)
    n = ks._n_values((6, 8), dev, 6)
    zeros = torch.zeros(6, dtype=torch.int32, device=dev)
    for causal in (True, False):
        want, want_lse = kg.shared_call(pkg, sh, q, n, causal)
        out, lse = pkg.flash_attention_n_kvcache_prefix_groups(q, sh.k, sh.v, sh.lens, sh.table, sh.prefix_table.view(1, -1), sh.plen, zeros,
                                                               softmax_n_param=n, is_causal=causal, return_lse=True)
        assert torch.equal(out, want) and torch.equal(lse, want_lse), f"G = 1 is not the shared-prefix call bit for bit (causal={causal})"


@pytest.mark.parametrize("D,dt,Sq", [(64, "fp16", 3), (128, "bf16", 1)])
def test_nobody_grouped_is_the_base_call(pkg, dev, D, dt, Sq):
    """every prefix_group entry out of range: P_b = 0 everywhere, no prefix partial is read; the prefix tables and lengths may hold anything"""
    dtype = DTYPES[dt]
    q, kd, vd = kg.data(dev, 7, 8, 2, Sq, D, dtype, PAGE, 5, 311)
    gr = kg.Groups(kd, vd, MIXED_LENS, [-1, 3, 99, -7, 2 ** 31 - 1, -2 ** 31, 3], MIXED_PLENS, PAGE, 5, 13, prefix_pages=4)
    assert (gr.prefix_tables == gr.poison).all() and gr.Pb == [0] * 7
    n = ks._n_values((7, 8), dev, 2)
    lens_junk = torch.tensor([2 ** 31 - 1, -5, 77], dtype=torch.int32, device=dev)
    for causal in (True, False):
        want, want_lse = pkg.flash_attention_n_kvcache(q, gr.k, gr.v, gr.lens, block_table=gr.table, softmax_n_param=n, is_causal=causal, return_lse=True)
        out, lse = kg.groups_call(pkg, gr, q, n, causal, prefix_lens=lens_junk)
        assert torch.equal(out, want) and torch.equal(lse, want_lse), f"nobody grouped is not the base call bit for bit (causal={causal})"


def test_out_of_range_groups_are_no_group_and_runs_repeat(pkg, dev):
    """G, -7 and 2^31 - 1 in prefix_group give the bits of -1; a second run gives the first run's bits"""
    dtype = torch.bfloat16
    q, kd, vd = kg.data(dev, 7, 8, 2, 3, 64, dtype, PAGE, 5, 321)
    gr = kg.Groups(kd, vd, MIXED_LENS, MIXED, MIXED_PLENS, PAGE, 5, 17, prefix_pages=4)
    n = ks._n_values((7, 8), dev, 5)
    want, want_lse = kg.groups_call(pkg, gr, q, n)
    kg.check(pkg, gr, want, want_lse, q, n, True, dtype, "the -1 run")
    for other in (3, -7, 2 ** 31 - 1):
        group = torch.tensor([g if g != -1 else other for g in MIXED], dtype=torch.int32, device=dev)
        out, lse = kg.groups_call(pkg, gr, q, n, prefix_group=group)
        assert torch.equal(out, want) and torch.equal(lse, want_lse), f"prefix_group = {other} is not 'no shared prefix'"
    again, again_lse = kg.groups_call(pkg, gr, q, n)
    assert torch.equal(again, want) and torch.equal(again_lse, want_lse), "a second run differs"


def test_prefix_lens_are_clamped_per_group(pkg, dev):
    """-5, 10000, -2^31 and 2^31 - 1 in the four groups of one call: 0, max_prefix_pages * page, 0, max_prefix_pages * page"""
    group = [0, 1, 2, 3, 1, 3, 0, 2]
    lens = [3 * PAGE + 1, 2 * PAGE, 37, 0, 2 * PAGE + 1, 4 * PAGE, 90, 129]
    q, kd, vd = kg.data(dev, 8, 8, 2, 4, 64, torch.bfloat16, PAGE, 5, 331)
    gr = kg.Groups(kd, vd, lens, group, (0, 2 * PAGE, 0, 2 * PAGE), PAGE, 5, 3, prefix_pages=2)
    n = ks._n_values((8, 8), dev, 9)
    raw = torch.tensor([-5, 10000, -2 ** 31, 2 ** 31 - 1], dtype=torch.int32, device=dev)
    out, lse = kg.groups_call(pkg, gr, q, n, True, prefix_lens=raw)
    kg.check(pkg, gr, out, lse, q, n, True, torch.bfloat16, "prefix_lens clamped per group")


@pytest.mark.parametrize("D,dt", [(64, "fp16"), (128, "bf16")])
def test_memory_contract(pkg, dev, D, dt):
    """what the contract lets hold anything holds NaN or points at the poison page - the table row of a group without a member and the
    own slots below P_b of a member whose group's prefix ends inside a page among it; the output is finite and passes the gates"""
    dtype = DTYPES[dt]
    group, plens = [2, 0, -1, 0, 2, 0, 3], (2 * PAGE + 37, 100, 70, 100)   # group 1 has no member; group 3 one, shorter than its prefix
    lens = [3 * PAGE + 1, 2 * PAGE + 37, 37, 0, 70, 4 * PAGE, 50]
    q, kd, vd = kg.data(dev, 7, 8, 2, 4, D, dtype, PAGE, 5, 341)
    gr = kg.Groups(kd, vd, lens, group, plens, PAGE, 5, 13, prefix_pages=4)
    tab, ptab = gr.table.cpu(), gr.prefix_tables.cpu()
    assert torch.isnan(gr.k[gr.poison]).all() and torch.isnan(gr.v[gr.poison]).all()
    assert (ptab[1] == gr.poison).all()                                               # the whole row of the group without a member
    for b, P in enumerate(gr.Pb):
        assert (tab[b, :P // PAGE] == gr.poison).all()                                # own slots wholly below P_b
    for g in (0, 2, 3):
        P = plens[g]
        assert (ptab[g, -(-P // PAGE):] == gr.poison).all() and ptab.shape[1] == 4   # prefix_tables[g] beyond ceil(P_g / page)
        last = int(ptab[g, P // PAGE])
        assert last != gr.poison and torch.isnan(gr.k[last, P % PAGE:]).all() and torch.isfinite(gr.k[last, :P % PAGE]).all()
    for b in (0, 5):                                                                  # own rows below P_b in the partially shared page
        P = gr.Pb[b]
        own = int(tab[b, P // PAGE])
        assert own != gr.poison and torch.isnan(gr.v[own, :P % PAGE]).all() and torch.isfinite(gr.v[own, P % PAGE]).all()
    assert torch.isnan(gr.k[int(tab[0, 3]), 1:]).all()                                # rows at or beyond len_b
    n = ks._n_values((7, 8), dev, 4)
    for causal in (True, False):
        out, lse = kg.groups_call(pkg, gr, q, n, causal)
        assert torch.isfinite(out).all() and not torch.isnan(lse).any()
        kg.check(pkg, gr, out, lse, q, n, causal, dtype, f"contract D={D} {dt} causal={causal}")


# ---------------------------------------------------------------- kv_witness behind three prefixes of one call
WITNESS_PLENS = (63, 64, 65)


@pytest.mark.parametrize("nkind", ["zero", "one", "tensor"])
@pytest.mark.parametrize("D,dt,Sq", [(64, "bf16", 1), (128, "fp16", 3)])
def test_every_key_once_and_the_sink_once(pkg, dev, D, dt, Sq, nkind):
    """kv_witness A: query 0 and indicator V - exp(lse) = n + visible keys, out Z counts the keys of a class. P = 63, 64, 65 in the three
    groups of one call, len_b on either side of each"""
    dtype = DTYPES[dt]
    lens = [40, 62, 63, 64, 65, 66, 130, 200, 0, 64, 65, 63]
    group = [0, 1, 2, 0, 1, 2, 0, 1, 2, -1, 0, 1]
    case = kg.witness_case(8, 2, D, Sq, lens)
    inp = kw.inputs_a(case, dtype, dev, 68)
    if nkind == "tensor":
        inp["n"] = ks._n_values((case.B, case.H), dev, 17)
        assert (inp["n"] == 0).any() and (inp["n"] > 0).any()
    else:
        inp["n"] = torch.tensor(0.0 if nkind == "zero" else 1.0, device=dev)
    got, seen = kg.groups_witness_run(pkg, case, inp, group, WITNESS_PLENS)
    refs = kw.reference(case, seen)
    kw.condition_a(refs, dtype)
    ratios = [kw.gate_a(o, lse, r) for (o, lse), r in zip(got, refs)]
    rz, ro = max(r[0] for r in ratios), max(r[1] for r in ratios)
    print(f"A n={nkind}: exp(lse) at {rz:.3g} of 1e-5 Z, out Z at {ro:.3g} of 0.25")
    assert rz <= 1, f"exp(lse) is {rz:.3g}x (1e-5 Z_ref) from n + the number of visible keys, per sequence {[r[0] for r in ratios]}"
    assert ro <= 1, f"out Z_ref is {ro:.3g}x 0.25 from the class counts, per sequence {[r[1] for r in ratios]}"


@pytest.mark.parametrize("form", kw.B_FORMS)
@pytest.mark.parametrize("D,dt,Sq", [(64, "fp16", 1), (128, "bf16", 3), (64, "bf16", 2)])
def test_one_key_decides(pkg, dev, D, dt, Sq, form):
    """kv_witness B, scale 32: the deciding key lies below P_b where len_b <= P_b and at or above it elsewhere; a partial merged with the
    wrong weight, or read at another sequence's slot, gives another key's V row"""
    dtype = DTYPES[dt]
    lens = [40, 63, 66, 62, 64, 65, 130, 200, 3, 0, 64, 67]
    group = [0, 1, 2, 0, 1, 2, -1, 1, 2, 0, 0, 1]
    case = kg.witness_case(8, 2, D, Sq, lens)
    inp = kw.inputs_b(case, form, dtype, dev, 23)
    got, seen = kg.groups_witness_run(pkg, case, inp, group, WITNESS_PLENS)
    refs = kw.reference(case, seen)
    ratios, kinds = [], set()
    for b, ((o, lse), r) in enumerate(zip(got, refs)):
        kind, want = kw.expect_b(r, kw.sequence(case, seen, b)[2][:, :case.total[b]], case.H // case.Hkv)
        kinds |= set(kind.unique().tolist())
        ratios.append(kw.gate_b(o, kind, want, dtype))
        ks._check_lse(lse, r["lse"].float(), f"B {form} sequence {b} lse")
    print(f"B {form} {dt}: out at {max(ratios):.3g} of its gate; row kinds {sorted(kinds)}")
    assert max(ratios) <= 1, f"out is {max(ratios):.3g}x the gate from the deciding key's V row, per sequence {ratios}"
    assert 1 in kinds or form == "sink"


# ---------------------------------------------------------------- the schedule table
def _table_of(pkg, dev, H, Hkv, Sq, group, G, plens, seed):
    """fasn_fwd_prefix_groups through the ctypes layer with a workspace of the test's own; the table at its documented offset"""
    B, D, max_pages = len(group), 64, 2
    rnd = random.Random(seed)
    lens = [rnd.randrange(0, PAGE * max_pages + 1) for _ in range(B)]
    q, kd, vd = kg.data(dev, B, H, Hkv, Sq, D, torch.float16, PAGE, max_pages, seed)
    gr = kg.Groups(kd, vd, lens, group, plens, PAGE, max_pages, seed, prefix_pages=2)
    lib = pkg._lib.load()
    c = pkg.kvcache._prepare("test", "kvcache", q, gr.k, gr.v, gr.lens, gr.table, None, None, 1.0, None, True, True)
    ops = pkg._lib.PrefixGroups(prefix_lens=gr.plens.data_ptr(), prefix_tables=gr.prefix_tables.data_ptr(), prefix_group=gr.group.data_ptr(),
                                num_groups=G, max_prefix_pages=2, reserved=0)
    need = lib.fasn_fwd_prefix_groups_workspace_bytes(c.args, ops)
    rule = kg.groups_plan_rule(B, H, Hkv, Sq, D, PAGE, max_pages, G, 2)
    assert need == rule[4]
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device=dev)
    pkg._lib.check(lib.fasn_fwd_prefix_groups(c.args, ops, ws.data_ptr(), need, pkg.kvcache._stream_ptr(dev)), "fasn_fwd_prefix_groups")
    torch.cuda.synchronize()
    assert torch.isfinite(c.out).all()
    return kg.read_table(ws, rule[3], B, (H // Hkv) * Sq, G)


@pytest.mark.parametrize("name", sorted(ASSIGNMENTS) + ["random300"])
def test_schedule_table_is_the_model(pkg, dev, name):
    if name == "random300":
        rnd = random.Random(300)
        H, Hkv, Sq, G = 8, 2, 1, 7
        group = [rnd.randrange(-2, G + 2) for _ in range(300)]
    else:
        H, Hkv, Sq, group, G = ASSIGNMENTS[name]
    plens = [(37 * g + 20) % 129 for g in range(G)]
    got = _table_of(pkg, dev, H, Hkv, Sq, group, G, plens, 11)
    want = kg.model(group, G, (H // Hkv) * Sq, plens)
    for what, g, w in zip(("order", "slots", "items", "P_b", "P_g of the items"), got, want):
        assert g == w, f"{name}: {what} differ from the model"


# ---------------------------------------------------------------- append, graph, refusals
@pytest.mark.parametrize("D,dt", [(64, "fp16"), (128, "bf16")])
def test_append(pkg, dev, D, dt):
    """k_new / v_new go to the sequence's own pages at cache_seqlens[b] + i: where that is at or beyond P_b they are attended to, where it
    is below (rows 90 .. 93 of b = 1 under P = 100, rows 64 .. 67 of b = 4 under P = 70) they are never read"""
    dtype, Sq, B = DTYPES[dt], 4, 6
    old, group, plens = [110, 90, 98, 100, 64, 68], [0, 0, -1, 0, 1, 1], (100, 70)
    q, kd, vd = kg.data(dev, B, 8, 2, Sq, D, dtype, PAGE, 4, 41)
    gr = kg.Groups(kd, vd, old, group, plens, PAGE, 4, 19, alloc_all=True)
    kn = torch.stack([gr.kd[b, :, old[b]:old[b] + Sq] for b in range(B)])
    vn = torch.stack([gr.vd[b, :, old[b]:old[b] + Sq] for b in range(B)])
    n = ks._n_values((B, 8), dev, 2)
    out, lse = kg.groups_call(pkg, gr, q, n, True, k_new=kn, v_new=vn)
    new = [ln + Sq for ln in old]
    kgath, vgath = gr.gather(new)
    assert torch.equal(kgath, ks._visible_dense(gr.kd, new)[:, :, :kgath.shape[2]]) and torch.equal(vgath, ks._visible_dense(gr.vd, new)[:, :, :vgath.shape[2]])
    kg.check(pkg, gr, out, lse, q, n, True, dtype, f"append D={D} {dt}", lens=new)


def test_one_graph_serves_every_assignment(pkg, dev):
    """captured once; prefix_group, prefix_lens, prefix_tables, cache_seqlens, block_table (and the cache) change in place: the replay is
    the eager call on the new contents"""
    dtype, B, H, Hkv, Sq, D = torch.bfloat16, 6, 8, 2, 2, 64
    builds = []
    for seed, group, plens, lens in ((1, [0, 1, 0, -1, 1, 2], (2 * PAGE + 37, 65, 10), [200, 165, 37, 0, 256, 9]),
                                     (2, [2, 2, 2, 2, 2, 2], (0, 0, 129), [130, 3, 190, 64, 65, 256]),
                                     (3, [-1, 5, 9, -3, 7, 3], (50, 60, 70), [1, 0, 256, 64, 100, 77]),
                                     (4, [1, -1, 0, 0, 1, 0], (64, 128, 0), [64, 100, 256, 65, 129, 0])):
        q, kd, vd = kg.data(dev, B, H, Hkv, Sq, D, dtype, PAGE, 4, 10 * seed)
        builds.append((q, kg.Groups(kd, vd, lens, group, plens, PAGE, 4, seed, prefix_pages=3, alloc_all=True)))
    n = ks._n_values((B, H), dev, 12)
    names = ("k", "v", "lens", "table", "prefix_tables", "plens", "group")
    q0, g0 = builds[0]
    static = {a: getattr(g0, a).clone() for a in names}
    qs = q0.clone()

    def run():
        return pkg.flash_attention_n_kvcache_prefix_groups(qs, static["k"], static["v"], static["lens"], static["table"], static["prefix_tables"],
                                                           static["plens"], static["group"], softmax_n_param=n, return_lse=True)
    g, (out, lse) = ks._capture(run)
    for q, gr in builds[::-1]:
        qs.copy_(q)
        for a in names:
            static[a].copy_(getattr(gr, a))
        g.replay()
        torch.cuda.synchronize()
        want, want_lse = kg.groups_call(pkg, gr, q, n, True)
        assert torch.equal(out, want) and torch.equal(lse, want_lse), f"replay differs from the eager call for groups {gr.group_list}"
        kg.check(pkg, gr, out, lse, q, n, True, dtype, f"graph groups={gr.group_list}")


def test_refusals_name_their_reason(pkg, dev):
    fa = pkg.flash_attention_n_kvcache_prefix_groups
    q, kd, vd = kg.data(dev, 2, 8, 2, 1, 64, torch.float16, PAGE, 3, 5)
    gr = kg.Groups(kd, vd, [70, 100], [0, 1], (64, 10), PAGE, 3, 1)
    args = (q, gr.k, gr.v, gr.lens, gr.table, gr.prefix_tables, gr.plens, gr.group)
    with pytest.raises(ValueError, match="a dense cache .block_table=None. is not supported"):
        fa(q, gr.k, gr.v, gr.lens, None, *args[5:])
    with pytest.raises(TypeError, match="a float8 cache is not supported"):
        fa(q, gr.k.to(torch.float8_e4m3fn), gr.v.to(torch.float8_e4m3fn), *args[3:])
    for D in (32, 256):
        with pytest.raises(ValueError, match=r"head dim %d is not supported behind shared prefixes \(supported: \(64, 128\)" % D):
            fa(q[..., :1].expand(-1, -1, -1, D), *args[1:])
    with pytest.raises(ValueError, match="rows exceed the 128 of one pass"):
        fa(torch.zeros(2, 8, 33, 64, dtype=torch.float16, device=dev), *args[1:])
    for bad in (gr.prefix_tables.long(), gr.prefix_tables[0], gr.prefix_tables[:0], gr.prefix_tables[:, ::2], [[1, 2]]):
        with pytest.raises(ValueError, match=r"prefix_tables must be a contiguous int32 tensor of shape .G, max_prefix_pages."):
            fa(*args[:5], bad, gr.plens, gr.group)
    with pytest.raises(ValueError, match="1025 prefix groups exceed the 1024 of one call"):
        fa(*args[:5], torch.zeros(1025, 3, dtype=torch.int32, device=dev), torch.zeros(1025, dtype=torch.int32, device=dev), gr.group)
    for bad in (gr.plens.long(), gr.plens.view(1, 2), 64, gr.plens.float()):
        with pytest.raises(ValueError, match=r"prefix_lens must be a contiguous int32 tensor of shape .G."):
            fa(*args[:6], bad, gr.group)
    with pytest.raises(ValueError, match="prefix_lens has 3 entries, prefix_tables 2 rows"):
        fa(*args[:6], torch.zeros(3, dtype=torch.int32, device=dev), gr.group)
    for bad in (gr.group.long(), gr.group.view(2, 1), [0, 1], gr.group.float()):
        with pytest.raises(ValueError, match=r"prefix_group must be a contiguous int32 tensor of shape .B."):
            fa(*args[:7], bad)
    with pytest.raises(ValueError, match="prefix_group has 3 entries, the batch 2 elements"):
        fa(*args[:7], torch.zeros(3, dtype=torch.int32, device=dev))
    for i, name in ((5, "prefix_tables"), (6, "prefix_lens"), (7, "prefix_group")):
        moved = list(args)
        moved[i] = moved[i].cpu()
        with pytest.raises(RuntimeError, match=f"{name} is on cpu"):
            fa(*moved)
    with pytest.raises(RuntimeError, match="forward only"):
        fa(q.clone().requires_grad_(), *args[1:])
    out = fa(*args)   # what is refused above is not this call's shape
    assert out.shape == q.shape and torch.isfinite(out).all()
