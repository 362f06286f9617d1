"""Decode behind several shared prefixes (fasn_fwd_prefix_groups), without a GPU: the operand's layout, the exports against the header and
the bindings, the validation codes and their order behind the base checks (fake, aligned pointers: validation comes before any HIP call),
the launch plans - equal to tests/golden/kvgroups_plans.txt and to the rule restated in tests/kv_prefix.py, at G = 1 the shared-prefix
call's plus the schedule launch and the table's bytes - the integer model of the schedule table, the register tables of the new kernels
and the front end's refusals."""
import ctypes
import inspect
import os
import random
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kv_args as ka     # noqa: E402
import kv_prefix as kg   # noqa: E402

DUMMY, BIG = ka.DUMMY, ka.BIG
NEW = ("fasn_fwd_prefix_groups_workspace_bytes", "fasn_fwd_prefix_groups", "fasn_prefix_groups_plan")
DIMS = (64, 128)
TAGS = {0: "fasn::f16_tag", 1: "fasn::bf16_tag"}
EINVAL, EDTYPE, EHEADDIM, EALIGN, ESTRIDE, EUNSUPPORTED, EWORKSPACE = -1, -2, -3, -4, -5, -7, -8
_groups = kg._groups


def test_symbols_are_exported_and_bound(pkg):
    lib = pkg._lib.load()
    for name in NEW:
        assert name in pkg._lib.EXPORTS and hasattr(lib, name) and getattr(lib, name).argtypes is not None
    assert [b[0] for b in pkg._lib._prefix_groups_bindings()] == list(NEW)
    assert lib.fasn_abi_version() == 6 and pkg._lib.FASN_ABI_VERSION == 6
    S = pkg._lib.PrefixGroups
    assert ctypes.sizeof(S) == 40
    assert (S.prefix_lens.offset, S.prefix_tables.offset, S.prefix_group.offset, S.num_groups.offset, S.max_prefix_pages.offset,
            S.reserved.offset) == (0, 8, 16, 24, 28, 32)
    # the families the other suites count keep their members: the new names belong to none of them
    assert len(list(pkg._lib._kv_bindings())) == 69 and len(list(pkg._lib._shared_prefix_bindings())) == 3
    for name in NEW:
        assert not any(s in name for s in ("kvcache", "kvprefill", "kvvarlen")) and not name.startswith("fasn_kv_")


def test_header_declares_what_is_bound(pkg):
    raw = open(os.path.join(ROOT, "include", "fasn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(fasn_[a-z0-9_]+)\s*\(", text))
    assert set(NEW) <= declared and declared == set(pkg._lib.EXPORTS)
    body = re.search(r"typedef struct fasn_prefix_groups \{(.*?)\} fasn_prefix_groups;", text, flags=re.S).group(1)
    names = [n for _t, n in re.findall(r"([a-z0-9_ ]+?[ *]+)([A-Za-z_]+)(?:\[\d+\])?;", body)]
    assert names == [f[0] for f in pkg._lib.PrefixGroups._fields_]
    assert "#define FASN_ABI_VERSION 6" in text
    assert f"#define FASN_PREFIX_GROUPS_MAX {kg.GROUPS_MAX}" in text and pkg._lib.FASN_PREFIX_GROUPS_MAX == kg.GROUPS_MAX >= 64
    assert "FASN_PREFIX_GROUPS_TABLE_OFFSET" in raw and "order: the batch element of slot s" in raw   # the table is documented


def _calls(lib):
    buf = ctypes.create_string_buffer(4096)

    def plan(a, g):
        rc = lib.fasn_prefix_groups_plan(a, g, buf, len(buf))
        return rc if rc < 0 else 0
    return {"fwd": lambda a, g: lib.fasn_fwd_prefix_groups(a, g, DUMMY, BIG, None), "plan": plan}


def test_validation_codes_and_their_order(pkg):
    lib = pkg._lib.load()
    make = ka._args_decode
    good = _groups(pkg)
    for how, call in _calls(lib).items():
        # every base code with a good and with a bad operand: the base block's rules come first, with their codes
        for g in (good, None, _groups(pkg, reserved=1), _groups(pkg, pages=0), _groups(pkg, G=0), _groups(pkg, lens=DUMMY + 2)):
            assert call(None, g) == EINVAL
            assert call(make(pkg, B=0), g) == EINVAL
            assert call(make(pkg, dtype=2), g) == EDTYPE
            assert call(make(pkg, D=96), g) == EHEADDIM
            assert call(make(pkg, page=48), g) == EUNSUPPORTED
            a = make(pkg)
            a.q.ptr = a.q.ptr + 2
            assert call(a, g) == EALIGN
            a = make(pkg)
            a.q.stride[3] = 2
            assert call(a, g) == ESTRIDE
            assert call(make(pkg, seqlens=None), g) == EINVAL
            assert call(make(pkg, H=64, Hkv=8, Sq=17), g) == EUNSUPPORTED      # the decode row limit is a base rule
        # then the call's own rules, in the documented order: paged, head dim, the operand, its alignment
        for g in (good, None, _groups(pkg, G=0), _groups(pkg, group=DUMMY + 2)):
            assert call(make(pkg, paged=False, page=8192), g) == EUNSUPPORTED
            assert call(make(pkg, D=32), g) == EUNSUPPORTED and call(make(pkg, D=256), g) == EUNSUPPORTED
        assert call(make(pkg), None) == EINVAL
        for member in ("lens", "tables", "group"):
            assert call(make(pkg), _groups(pkg, **{member: None})) == EINVAL
        assert call(make(pkg), _groups(pkg, G=0)) == EINVAL and call(make(pkg), _groups(pkg, G=-1)) == EINVAL
        assert call(make(pkg), _groups(pkg, G=kg.GROUPS_MAX + 1)) == EINVAL and call(make(pkg), _groups(pkg, G=2 ** 31 - 1)) == EINVAL
        assert call(make(pkg), _groups(pkg, pages=0)) == EINVAL and call(make(pkg), _groups(pkg, pages=-3)) == EINVAL
        assert call(make(pkg), _groups(pkg, reserved=1)) == EINVAL
        assert call(make(pkg), _groups(pkg, reserved=1, lens=DUMMY + 2)) == EINVAL   # (reserved comes before the alignment)
        assert call(make(pkg), _groups(pkg, G=kg.GROUPS_MAX + 1, group=DUMMY + 2)) == EINVAL
        for member in ("lens", "tables", "group"):
            assert call(make(pkg), _groups(pkg, **{member: DUMMY + 2})) == EALIGN
        if how == "plan":   # (accepted arguments are only ever recorded, never launched)
            for G in (1, 2, 64, kg.GROUPS_MAX):
                assert call(make(pkg), _groups(pkg, G=G)) == 0
            for pages in (1, 33, 2 ** 31 - 1):
                assert call(make(pkg), _groups(pkg, pages=pages)) == 0
            assert call(make(pkg, D=128, dtype=0, H=8, Hkv=8, Sq=128), good) == 0
    ws = lib.fasn_fwd_prefix_groups_workspace_bytes
    assert ws(None, good) == 0 and ws(make(pkg), None) == 0 and ws(make(pkg, D=32), good) == 0 and ws(make(pkg, paged=False, page=8192), good) == 0
    assert ws(make(pkg), _groups(pkg, reserved=2)) == 0 and ws(make(pkg), _groups(pkg, tables=DUMMY + 2)) == 0
    assert ws(make(pkg), _groups(pkg, G=kg.GROUPS_MAX + 1)) == 0
    # then the workspace: missing, too small, misaligned
    a = make(pkg)
    need = ws(a, good)
    assert need > lib.fasn_fwd_kvcache_workspace_bytes(a) > 0
    assert lib.fasn_fwd_prefix_groups(a, good, DUMMY, need - 1, None) == EWORKSPACE
    assert lib.fasn_fwd_prefix_groups(a, good, None, need, None) == EWORKSPACE
    assert lib.fasn_fwd_prefix_groups(a, good, DUMMY + 4, need, None) == EALIGN
    assert lib.fasn_fwd_prefix_groups(a, None, None, 0, None) == EINVAL          # (the operand before the workspace)
    buf = ctypes.create_string_buffer(4096)
    assert lib.fasn_prefix_groups_plan(a, good, None, 10) == EINVAL and lib.fasn_prefix_groups_plan(a, good, buf, 8) == EINVAL


# ---------------------------------------------------------------- plans
def _expected_plan(tag, D, rule):
    gp, gs, gc = rule[:3]
    return [("fasn_kvgroups_schedule_kernel<256>", 1, 256, 0), (f"fasn_kvgroups_prefix_kernel<{tag}>", gp, 256, kg.lds_bytes(D)),
            (f"fasn_kvgroups_suffix_kernel<{tag}>", gs, 256, kg.lds_bytes(D)), (f"fasn_kvgroups_combine_kernel<{tag}>", gc, 256, 0)]


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("case", sorted(kg.GROUPS_PLAN_CASES))
def test_plan_and_workspace_follow_the_rule(pkg, case, D, dtype):
    """four launches; the grids, the LDS and the workspace as include/fasn.h states them, recomputed in Python; the suffix pass and the
    combine have the base call's grids"""
    shape, G, pages = kg.GROUPS_PLAN_CASES[case]
    lib = pkg._lib.load()
    args = lambda **kw: ka._args_decode(pkg, dtype=dtype, D=D, **dict(shape, **kw))   # noqa: E731
    plan = pkg._lib.prefix_groups_plan(args(), _groups(pkg, G=G, pages=pages))
    rule = kg.groups_plan_rule(D=D, G=G, prefix_pages=pages, **shape)
    assert plan == _expected_plan("%s, %d" % (TAGS[dtype], D), D, rule)
    base = pkg._lib.kvcache_plan(args())
    assert plan[2][1:] == base[0][1:] and plan[3][1:] == base[1][1:]
    assert lib.fasn_fwd_prefix_groups_workspace_bytes(args(), _groups(pkg, G=G, pages=pages)) == rule[4]
    assert rule[3] % 8 == 0 and rule[4] % 16 == 0


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("case", sorted(kg.SHARED_PLAN_CASES))
def test_one_group_plans_as_the_shared_prefix_call(pkg, case, D):
    """G = 1: kv_prefix.shared_plan_rule's grids and partial bytes, plus the schedule launch and the table's bytes"""
    shape, pages = kg.SHARED_PLAN_CASES[case]
    lib = pkg._lib.load()
    a = ka._args_decode(pkg, D=D, **shape)
    gp, gs, gc, partials = kg.shared_plan_rule(D=D, prefix_pages=pages, **shape)
    rule = kg.groups_plan_rule(D=D, G=1, prefix_pages=pages, **shape)
    assert rule[:4] == (gp, gs, gc, partials)
    one = pkg._lib.prefix_groups_plan(a, _groups(pkg, G=1, pages=pages))
    shared = pkg._lib.shared_prefix_plan(a, kg._prefix(pkg, pages=pages))
    assert one[0] == ("fasn_kvgroups_schedule_kernel<256>", 1, 256, 0)
    assert [k[1:] for k in one[1:]] == [k[1:] for k in shared]
    assert [k[0].replace("kvgroups", "kvshared") for k in one[1:]] == [k[0] for k in shared]
    R = (shape["H"] // shape["Hkv"]) * shape["Sq"]
    table = 4 * (4 + -(-3 * shape["B"] // 4) * 4 + 4 * -(-shape["B"] * R // 128))
    assert lib.fasn_fwd_prefix_groups_workspace_bytes(a, _groups(pkg, G=1, pages=pages)) == (partials + 15) // 16 * 16 + table
    assert lib.fasn_fwd_shared_prefix_workspace_bytes(a, kg._prefix(pkg, pages=pages)) == partials


def test_grids_do_not_depend_on_device_memory(pkg):
    """other lengths, another block table, other prefix tables, lengths and groups (other device pointers), an append: the same launches"""
    lib = pkg._lib.load()
    for case, (shape, G, pages) in kg.GROUPS_PLAN_CASES.items():
        a = ka._args_decode(pkg, **shape)
        plan = pkg._lib.prefix_groups_plan(a, _groups(pkg, G=G, pages=pages))
        other = ka._args_decode(pkg, seqlens=DUMMY + 4096, **shape)
        other.block_table = DUMMY + 65536
        other.seqlen_add = shape["Sq"]
        other.causal = 0
        moved = _groups(pkg, G=G, pages=pages, lens=DUMMY + 2048, tables=DUMMY + 4096, group=DUMMY + 8192)
        assert pkg._lib.prefix_groups_plan(other, moved) == plan, case
        assert lib.fasn_fwd_prefix_groups_workspace_bytes(other, moved) == lib.fasn_fwd_prefix_groups_workspace_bytes(a, _groups(pkg, G=G, pages=pages))


def _plan_text(pkg):
    lib = pkg._lib.load()
    got = []
    for D in DIMS:
        for dtype in (0, 1):
            for name in sorted(kg.GROUPS_PLAN_CASES):
                shape, G, pages = kg.GROUPS_PLAN_CASES[name]
                buf = ctypes.create_string_buffer(4096)
                rc = lib.fasn_prefix_groups_plan(ka._args_decode(pkg, dtype=dtype, D=D, **shape), _groups(pkg, G=G, pages=pages), buf, len(buf))
                assert rc > 0, (name, D, dtype, rc)
                got += [f"{name} {line}" for line in buf.value.decode().splitlines()]
    return got


def test_plans_equal_the_golden_file(pkg, golden_dir):
    want = open(os.path.join(golden_dir, "kvgroups_plans.txt")).read().splitlines()
    assert _plan_text(pkg) == want


# ---------------------------------------------------------------- the integer model of the schedule table
@pytest.mark.parametrize("seed", range(12))
def test_model_serves_every_row_once(seed):
    """random assignments: every row of every grouped sequence is in exactly one item, no item mixes groups, the item count is within
    items_max (the bound the grid is sized by), the order is stable"""
    rnd = random.Random(seed)
    B, G = rnd.choice([1, 2, 7, 40, 129, 300, 1000]), rnd.choice([1, 2, 3, 7, 64, kg.GROUPS_MAX])
    R = rnd.choice([1, 2, 4, 12, 15, 64, 128])
    spread = rnd.choice([G, max(1, G // 8), 2])   # how many groups are in use: many small ones, or a few large
    group = [rnd.choice([-1, G, -7, 2 ** 31 - 1]) if rnd.random() < 0.2 else rnd.randrange(spread) for _ in range(B)]
    order, slot, items, _, _ = kg.model(group, G, R)
    grouped = [b for b in range(B) if 0 <= group[b] < G]
    assert len(items) <= kg.items_max(B, R, G)
    assert sorted(order[:len(grouped)]) == grouped and order[len(grouped):] == [-1] * (B - len(grouped))
    keys = [(group[b], b) for b in order[:len(grouped)]]
    assert keys == sorted(keys), "not sorted by group, inside a group by batch index"
    assert all((slot[b] >= 0) == (b in set(grouped)) for b in range(B)) and all(order[slot[b]] == b for b in grouped)
    served = [0] * (len(grouped) * R)
    for g, row0, rend in items:
        assert row0 < rend
        for row in range(row0, min(row0 + kg.ROWS, rend)):
            served[row] += 1
            assert group[order[row // R]] == g, "an item mixes groups"
    assert served == [1] * len(served)


def test_items_max_is_reached_and_never_exceeded():
    """k groups of one row more than a multiple of 128: the bound's worst case"""
    for B, R, G in ((64, 1, 64), (40, 4, 2), (130, 1, 3), (300, 15, 7)):
        best = 0
        for k in range(1, min(G, B) + 1):
            sizes = [1] * (k - 1) + [B - (k - 1)]
            group = [g for g, c in enumerate(sizes) for _ in range(c)]
            best = max(best, len(kg.model(group, G, R)[2]))
            assert len(kg.model(group, G, R)[2]) <= kg.items_max(B, R, G)
        assert best >= -(-B * R // 128)


# ---------------------------------------------------------------- the kernels
def test_new_kernels_do_not_spill(pkg):
    """the schedule kernel and 3 kernels x 2 dtypes x 2 head dims = 13: each present once, spill 0, scratch 0"""
    import spill_map
    lib = os.path.join(ROOT, "flash-attention-softmax-n_amd", "libfasn.so")
    if not os.path.exists(spill_map.READELF):
        pytest.skip("llvm-readelf not available")
    table = spill_map.kernel_table(lib)
    names = sorted(table)
    pretty = subprocess.run([spill_map.CXXFILT], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    by_pretty = dict(zip(pretty, names))
    wanted = set()
    for D in DIMS:
        for dtype in (0, 1):
            shape, G, pages = kg.GROUPS_PLAN_CASES["straddle"]
            wanted |= {k[0] for k in pkg._lib.prefix_groups_plan(ka._args_decode(pkg, dtype=dtype, D=D, **shape), _groups(pkg, G=G, pages=pages))}
    assert len(wanted) == 13, wanted
    for name in sorted(wanted):
        hit = [m for d, m in by_pretty.items() if d.startswith("void fasn::" + name + "(")]
        assert len(hit) == 1, (name, hit)
        v = table[hit[0]]
        assert v.get("spill", 0) == 0 and v.get("scratch", 0) == 0, (name, v)
    assert sum("kvgroups" in d for d in by_pretty) == 13


def test_no_new_spill_allowance(golden_dir):
    import json
    allowance = json.load(open(os.path.join(golden_dir, "spill_allowance.json")))
    assert not [k for k in map(str, allowance if isinstance(allowance, (list, dict)) else []) if "kvgroups" in k or "prefix_groups" in k]


# ---------------------------------------------------------------- front end on CPU tensors
def test_front_end_refuses_with_the_reason(pkg):
    fa = pkg.flash_attention_n_kvcache_prefix_groups
    B, H, Hkv = 2, 8, 2
    q = torch.zeros(B, H, 4, 64, dtype=torch.float16)
    kc = torch.zeros(6, 64, Hkv, 64, dtype=torch.float16)
    sl = torch.zeros(B, dtype=torch.int32)
    bt = torch.zeros(B, 2, dtype=torch.int32)
    pt = torch.zeros(3, 2, dtype=torch.int32)
    pl = torch.zeros(3, dtype=torch.int32)
    pg = torch.zeros(B, dtype=torch.int32)
    with pytest.raises(ValueError, match="a dense cache .block_table=None. is not supported: a shared prefix is a set of pages"):
        fa(q, kc, kc, sl, None, pt, pl, pg)
    with pytest.raises(TypeError, match="a float8 cache is not supported .fp16 and bf16 caches only"):
        fa(q, kc.to(torch.float8_e4m3fn), kc.to(torch.float8_e4m3fn), sl, bt, pt, pl, pg)
    for D in (32, 256):
        with pytest.raises(ValueError, match=r"head dim %d is not supported behind shared prefixes \(supported: \(64, 128\)" % D):
            fa(torch.zeros(B, H, 4, D, dtype=torch.float16), torch.zeros(6, 64, Hkv, D, dtype=torch.float16), kc, sl, bt, pt, pl, pg)
    with pytest.raises(ValueError, match="head dim 96 is not supported"):
        fa(torch.zeros(B, H, 4, 96, dtype=torch.float16), kc, kc, sl, bt, pt, pl, pg)
    with pytest.raises(ValueError, match=r"4 x 33 = 132 rows exceed the 128 of one pass"):
        fa(torch.zeros(B, H, 33, 64, dtype=torch.float16), kc, kc, sl, bt, pt, pl, pg)
    for bad in (pt.long(), pt[0], pt[:0], pt[:, :0], torch.zeros(3, 4, dtype=torch.int32)[:, ::2], [[0, 1]], None):
        with pytest.raises(ValueError, match=r"prefix_tables must be a contiguous int32 tensor of shape .G, max_prefix_pages. on the device"):
            fa(q, kc, kc, sl, bt, bad, pl, pg)
    with pytest.raises(ValueError, match="1025 prefix groups exceed the 1024 of one call"):
        fa(q, kc, kc, sl, bt, torch.zeros(1025, 2, dtype=torch.int32), torch.zeros(1025, dtype=torch.int32), pg)
    for bad in (pl.long(), pl.view(1, 3), torch.zeros(6, dtype=torch.int32)[::2], 64, None):
        with pytest.raises(ValueError, match=r"prefix_lens must be a contiguous int32 tensor of shape .G. on the device"):
            fa(q, kc, kc, sl, bt, pt, bad, pg)
    for n in (1, 2, 4):
        with pytest.raises(ValueError, match=f"prefix_lens has {n} entries, prefix_tables 3 rows: one length per prefix"):
            fa(q, kc, kc, sl, bt, pt, torch.zeros(n, dtype=torch.int32), pg)
    for bad in (pg.long(), pg.view(1, B), torch.zeros(2 * B, dtype=torch.int32)[::2], [0, 0], None):
        with pytest.raises(ValueError, match=r"prefix_group must be a contiguous int32 tensor of shape .B. on the device"):
            fa(q, kc, kc, sl, bt, pt, pl, bad)
    for n in (1, 3):
        with pytest.raises(ValueError, match=f"prefix_group has {n} entries, the batch 2 elements: one group per batch element"):
            fa(q, kc, kc, sl, bt, pt, pl, torch.zeros(n, dtype=torch.int32))
    for i, name in ((5, "prefix_tables"), (6, "prefix_lens"), (7, "prefix_group")):
        moved = [q, kc, kc, sl, bt, pt, pl, pg]
        moved[i] = moved[i].to("meta")
        with pytest.raises(RuntimeError, match=f"{name} is on meta"):
            fa(*moved)
    with pytest.raises(RuntimeError, match="forward only"):
        fa(q.clone().requires_grad_(), kc, kc, sl, bt, pt, pl, pg)
    with pytest.raises(RuntimeError, match="forward only"):
        fa(q, kc, kc, sl, bt, pt, pl, pg, softmax_n_param=torch.ones(H, requires_grad=True))
    # the base call keeps refusing what it refuses
    with pytest.raises(ValueError, match="int32"):
        fa(q, kc, kc, sl.long(), bt, pt, pl, pg)
    with pytest.raises(ValueError, match="k_new and v_new come together"):
        fa(q, kc, kc, sl, bt, pt, pl, pg, k_new=torch.zeros(B, Hkv, 4, 64, dtype=torch.float16))
    # a valid call gets as far as the CPU-tensor refusal, with and without new rows
    kn = torch.zeros(B, Hkv, 4, 64, dtype=torch.float16)
    for new in ({}, dict(k_new=kn, v_new=kn)):
        with pytest.raises(RuntimeError, match="device tensors only"):
            fa(q, kc, kc, sl, bt, pt, pl, pg, **new)


def test_signature_and_membership(pkg):
    fa = pkg.flash_attention_n_kvcache_prefix_groups
    assert "flash_attention_n_kvcache_prefix_groups" in pkg.__all__ and "flash_attention_n_kvcache_prefix_groups" in pkg.__doc__
    assert pkg.kvcache.flash_attention_n_kvcache_prefix_groups is fa
    sig = inspect.signature(fa)
    assert list(sig.parameters) == ["query", "k_cache", "v_cache", "cache_seqlens", "block_table", "prefix_tables", "prefix_lens", "prefix_group",
                                    "k_new", "v_new", "softmax_n_param", "scale", "is_causal", "return_lse"]
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(k_new=None, v_new=None, softmax_n_param=1, scale=None, is_causal=True, return_lse=False)
    assert pkg._lib.prefix_groups_plan.__doc__ and "prefix_group" in fa.__doc__
    # the single-prefix call keeps its signature and its messages
    old = inspect.signature(pkg.flash_attention_n_kvcache_shared_prefix)
    assert list(old.parameters)[5:7] == ["prefix_table", "prefix_len"]
