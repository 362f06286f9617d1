"""flash_attention_n_kvcache_varlen / fasn_fwd_kvvarlen without a GPU: the front end's refusals (CPU tensors: the argument checks come
before the device check), the order of the C ABI's checks (tests/golden/kvvarlen_host_matrix.txt, in the style of kvhost_matrix.txt), the
recorded launch plans (tests/golden/kvvarlen_plans.txt), the registers of the new kernels, and a pure-Python mirror of the schedule
kernel, which tests/test_gpu_kvvarlen.py reuses.

Nothing is ever launched: the pointers are fake. Valid blocks go through fasn_kvvarlen_plan and fasn_fwd_kvvarlen_workspace_bytes only
(and through fasn_kvvarlen_append with NULL rows, which is refused behind the block's checks); the forward is called only with blocks the
plan call has just refused.

    python tests/test_kvvarlen_cpu.py --record     rewrites both fixtures from the library of this tree
"""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kv_args as ka   # noqa: E402

DUMMY, BIG = ka.DUMMY, ka.BIG
_args, items_max, plan_cases = ka._args_varlen, ka.items_max, ka.plan_cases
MATRIX = os.path.join(ROOT, "tests", "golden", "kvvarlen_host_matrix.txt")
PLANS = os.path.join(ROOT, "tests", "golden", "kvvarlen_plans.txt")


# ---------------------------------------------------------------- the schedule, mirrored
def schedule(cu, max_seqlen_q, T, PB):
    """fasn_kvvarlen_schedule_kernel in Python: [(b, rb, token0, qlen)], sequences in order, the last row block of a sequence first,
    cut at items_max"""
    items = []
    for b in range(len(cu) - 1):
        token0 = min(max(cu[b], 0), T)
        qlen = min(min(max(cu[b + 1] - cu[b], 0), max_seqlen_q), T - token0)
        nblk = -(-qlen // PB)
        items += [(b, nblk - 1 - j, token0, qlen) for j in range(nblk)]
    return items[:items_max(len(cu) - 1, max_seqlen_q, T, PB)]


RAGGED = [
    ([1, 0, 16, 17, 35, 1], 40, 7), ([1, 1, 1, 1], 48, 60), ([48, 0, 0, 16], 48, 0), ([0, 0, 0], 5, 3), ([2048] + [1] * 255, 4096, 2049),
    ([1] * 256, 1, 0), ([2048] * 4, 2048, 0), ([127, 129, 128], 129, 1),
]


@pytest.mark.parametrize("PB", [1, 16, 42, 128])
@pytest.mark.parametrize("case", range(len(RAGGED)))
def test_schedule_mirror_covers_every_token_once(case, PB):
    qlens, max_q, tail = RAGGED[case]
    cu = [0]
    for ql in qlens:
        cu.append(cu[-1] + ql)
    T = cu[-1] + tail
    items = schedule(cu, max_q, T, PB)
    assert len(items) <= items_max(len(qlens), max_q, T, PB)
    assert len(items) == sum(-(-ql // PB) for ql in qlens)          # well-formed offsets: the bound never cuts
    seen = [0] * T
    last = {}
    for b, rb, token0, qlen in items:
        assert 0 <= b < len(qlens) and token0 == cu[b] and qlen == qlens[b] and 0 <= rb * PB < qlen
        assert last.get(b, rb + 1) == rb + 1, "within a sequence the last row block comes first, then downwards"
        last[b] = rb
        for pos in range(rb * PB, min(rb * PB + PB, qlen)):
            seen[token0 + pos] += 1
    assert seen == [1] * cu[-1] + [0] * tail


# ---------------------------------------------------------------- the front end
def test_front_end_refuses_with_the_reason(pkg):
    fa = pkg.flash_attention_n_kvcache_varlen
    import flash_attention_softmax_n_amd as shim
    assert shim.flash_attention_n_kvcache_varlen is fa and "flash_attention_n_kvcache_varlen" in pkg.__all__
    f16 = torch.float16
    q = torch.zeros(10, 8, 64, dtype=f16)
    kc = torch.zeros(4, 64, 2, 64, dtype=f16)
    sl = torch.zeros(2, dtype=torch.int32)
    cu = torch.tensor([0, 4, 9], dtype=torch.int32)
    bt = torch.zeros(2, 2, dtype=torch.int32)
    kn = torch.zeros(10, 2, 64, dtype=f16)
    with pytest.raises(RuntimeError, match="CPU tensor"):      # arguments that are right get as far as the device check
        fa(q, kc, kc, sl, cu, 8, block_table=bt)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        fa(q, kc, kc, sl, cu, 8, block_table=bt, k_new=kn, v_new=kn, softmax_n_param=torch.ones(2, 8), return_lse=True)
    with pytest.raises(RuntimeError, match="CPU tensor"):      # a bound beyond the buffer is a bound
        fa(q, kc, kc, sl, cu, 1 << 20, block_table=bt)
    # query
    for bad in (torch.zeros(2, 8, 5, 64, dtype=f16), torch.zeros(10, 64, dtype=f16)):
        with pytest.raises(ValueError, match=r"query must be token-packed \[T, H, D\]"):
            fa(bad, kc, kc, sl, cu, 8, block_table=bt)
    # cu_seqlens_q
    for bad in (cu.long(), cu.view(3, 1), torch.zeros(6, dtype=torch.int32)[::2], [0, 4, 9], torch.zeros(1, dtype=torch.int32)):
        with pytest.raises(ValueError, match=r"cu_seqlens_q must be a contiguous int32 tensor of shape \[B \+ 1\]"):
            fa(q, kc, kc, sl, bad, 8, block_table=bt)
    with pytest.raises(RuntimeError, match="cu_seqlens_q is on meta, query on cpu"):
        fa(q, kc, kc, sl, cu.to("meta"), 8, block_table=bt)
    # B
    with pytest.raises(ValueError, match="cu_seqlens_q names 3 sequences but cache_seqlens has 2"):
        fa(q, kc, kc, sl, torch.tensor([0, 4, 9, 9], dtype=torch.int32), 8, block_table=bt)
    with pytest.raises(ValueError, match="block_table has 3 rows but the batch is 2"):
        fa(q, kc, kc, sl, cu, 8, block_table=torch.zeros(3, 2, dtype=torch.int32))
    # max_seqlen_q
    for bad in (8.0, torch.tensor(8), True, None):
        with pytest.raises(TypeError, match="max_seqlen_q must be a Python int"):
            fa(q, kc, kc, sl, cu, bad, block_table=bt)
    with pytest.raises(ValueError, match="max_seqlen_q must be >= 1; got 0"):
        fa(q, kc, kc, sl, cu, 0, block_table=bt)
    # k_new / v_new: token-packed like query
    with pytest.raises(ValueError, match="k_new and v_new come together"):
        fa(q, kc, kc, sl, cu, 8, block_table=bt, k_new=kn)
    for bad in (torch.zeros(2, 2, 5, 64, dtype=f16), torch.zeros(9, 2, 64, dtype=f16), torch.zeros(10, 8, 64, dtype=f16), kn.bfloat16()):
        with pytest.raises(ValueError, match=r"k_new must be \[T, Hkv, D\] = \[10, 2, 64\]"):
            fa(q, kc, kc, sl, cu, 8, block_table=bt, k_new=bad, v_new=bad)
    # tensor n: per sequence and head, not per token
    for bad in (torch.ones(10, 8), torch.ones(3, 8), torch.ones(2, 8, 1)):
        with pytest.raises(ValueError, match=r"softmax_n_param must broadcast to \[B, H\] = \[2, 8\]"):
            fa(q, kc, kc, sl, cu, 8, block_table=bt, softmax_n_param=bad)
    # what the packed call does not do yet is refused, not ignored
    for kw in (dict(alibi_slopes=torch.ones(8)), dict(window=128), dict(rotary_cos=torch.ones(128, 16)), dict(rotary_sin=torch.ones(128, 16))):
        with pytest.raises(NotImplementedError, match=f"{list(kw)[0]} is not supported on token-packed queries"):
            fa(q, kc, kc, sl, cu, 8, block_table=bt, **kw)
    # _prepare's refusals carry over
    with pytest.raises(ValueError, match="head dim 96"):
        k96 = torch.zeros(4, 64, 2, 96, dtype=f16)
        fa(torch.zeros(10, 8, 96, dtype=f16), k96, k96, sl, cu, 8, block_table=bt)
    with pytest.raises(ValueError, match="fp16 and bf16"):
        fa(q.float(), kc.float(), kc.float(), sl, cu, 8, block_table=bt)
    with pytest.raises(ValueError, match="page_size 16"):
        k16 = torch.zeros(4, 16, 2, 64, dtype=f16)
        fa(q, k16, k16, sl, cu, 8, block_table=bt)
    with pytest.raises(ValueError, match="query heads per K/V head"):
        k1 = torch.zeros(4, 64, 1, 64, dtype=f16)
        fa(torch.zeros(10, 256, 64, dtype=f16), k1, k1, sl, cu, 8, block_table=bt)
    with pytest.raises(RuntimeError, match="flash_attention_n_kvcache_varlen is forward only"):
        fa(q.clone().requires_grad_(), kc, kc, sl, cu, 8, block_table=bt)


def test_args_struct_extends_the_prefill_struct(pkg):
    L = pkg._lib
    assert L.KvVarlenArgs.pf.offset == 0 and L.KvVarlenArgs.pf.size == ctypes.sizeof(L.KvPrefillArgs)
    assert L.KvVarlenArgs.cu_seqlens_q.offset == ctypes.sizeof(L.KvPrefillArgs)
    assert ctypes.sizeof(L.KvVarlenArgs) == ctypes.sizeof(L.KvPrefillArgs) + 16
    assert L.load().fasn_abi_version() == 6


# ---------------------------------------------------------------- the order of the C ABI's checks
BASES = ("pre_paged_qlens", "pre_dense_oddpage", "d256")
PACKED_RULES = [
    ("cu_null", lambda c: setattr(c, "cu", None)), ("q_seqlens_set", ka._attr("qlens", DUMMY + 4096)), ("tokens_0", lambda c: setattr(c, "T", 0)),
    ("reserved_1", lambda c: setattr(c, "reserved", 1)), ("cu_odd", lambda c: setattr(c, "cu", DUMMY + 2)),
    ("table_over", lambda c: (setattr(c.kv, "B", 1 << 22), setattr(c.kv, "Sq", 1), setattr(c.kv, "seqlen_add", 1), setattr(c, "T", 1 << 28))),
]
CHAIN = ka.BASE_RULES + PACKED_RULES


def matrix_cases():
    out = [(name, name, ()) for name in BASES]
    for base in BASES:
        out += [(f"{base}+{n}", base, (fn,)) for n, fn in CHAIN]
    out += [(f"{BASES[0]}+{n1}+{n2}", BASES[0], (f1, f2)) for (n1, f1), (n2, f2) in zip(CHAIN, CHAIN[1:])]
    return out


def _matrix_line(pkg, name, base, rules):
    L, lib = pkg._lib, pkg._lib.load()
    c = ka.Case(L, dict(ka.BASES[base], qlens=False))
    c.cu, c.T, c.reserved = DUMMY + 8192, 3 * c.kv.Sq + 5, 0
    for rule in rules:
        rule(c)
    va = L.KvVarlenArgs()
    va.pf = c.pa
    va.pf.q_seqlens = c.qlens
    va.cu_seqlens_q, va.total_tokens, va.reserved = c.cu, c.T, c.reserved
    args = None if c.null else va
    plan = ka._plan(lib.fasn_kvvarlen_plan, args)
    got = [plan, str(lib.fasn_fwd_kvvarlen_workspace_bytes(args))]
    if plan.startswith("-"):   # the block itself is refused: the calls that would launch return the same way, before any HIP call
        got.append(f"fwd={lib.fasn_fwd_kvvarlen(args, 256, BIG, None)},{lib.fasn_kvvarlen_append(args, c.kn, c.vn, None)}")
    else:                      # accepted: the workspace and the rows are checked behind the block, still before any HIP call
        got.append(f"ws={lib.fasn_fwd_kvvarlen(args, None, BIG, None)},{lib.fasn_fwd_kvvarlen(args, 256, 8, None)},{lib.fasn_fwd_kvvarlen(args, 260, BIG, None)}"
                   f" rows={lib.fasn_kvvarlen_append(args, None, c.vn, None)}")
    return f"{name} | {' '.join(got)}"


def matrix(pkg):
    return [_matrix_line(pkg, *case) for case in matrix_cases()]


def test_return_codes_equal_the_recorded_matrix(pkg):
    want = open(MATRIX).read().splitlines()
    got = matrix(pkg)
    assert len(got) == len(want) == len(matrix_cases())
    diff = [(g, w) for g, w in zip(got, want) if g != w]
    assert not diff, f"{len(diff)} of {len(got)} cases moved; the first (got, recorded): {diff[:3]}"
    rows = dict(line.split(" | ", 1) for line in got)
    for base in BASES:   # the blocks the rules are broken on are accepted; a workspace is always asked for, NULL / short / misaligned refused
        assert rows[base].startswith("#") and " ws=-8,-8,-4 rows=-1" in rows[base] and int(rows[base].split()[1]) > 0, rows[base]
        for rule, code in (("cu_null", -1), ("q_seqlens_set", -1), ("tokens_0", -1), ("reserved_1", -1), ("cu_odd", -4), ("table_over", -1)):
            assert rows[f"{base}+{rule}"] == f"{code} 0 fwd={code},{code}", (base, rule, rows[f"{base}+{rule}"])


# ---------------------------------------------------------------- launch plans
def plan_lines(pkg):
    lib = pkg._lib.load()
    got = []
    for name, c in sorted(plan_cases().items()):
        va = _args(pkg, **c)
        buf = ctypes.create_string_buffer(4096)
        rc = lib.fasn_kvvarlen_plan(va, buf, len(buf))
        assert rc > 0, (name, rc)
        got += [f"{name} {line}" for line in buf.value.decode().splitlines()]
        got.append(f"{name} workspace={lib.fasn_fwd_kvvarlen_workspace_bytes(va)}")
    return got


def test_launch_plans_equal_the_recorded_ones(pkg):
    assert plan_lines(pkg) == open(PLANS).read().splitlines()


@pytest.mark.parametrize("case", sorted(plan_cases()))
def test_plan_follows_the_item_table(pkg, case):
    c = plan_cases()[case]
    lib = pkg._lib.load()
    va = _args(pkg, **c)
    plan = pkg._lib.kvvarlen_plan(va)
    names = [k[0] for k in plan]
    tag = "fasn::bf16_tag, %d" % c["D"]
    PB = 128 // (c["H"] // c["Hkv"])
    blocks = items_max(c["B"], c["Sq"], c["T"], PB) * c["Hkv"]
    assert names[:2] == ["fasn_kvvarlen_schedule_kernel<256>", f"fasn_kvvarlen_fwd_kernel<{tag}>"] and plan[0][1:] == (1, 256, 0)
    nsplit = plan[1][1] // blocks
    assert plan[1][1] == blocks * nsplit and (nsplit > 1) == case.endswith("small")
    assert names[2:] == ([f"fasn_kvvarlen_combine_kernel<{tag}>"] if nsplit > 1 else [])     # one split: no combine launch
    table = 16 + 16 * (blocks // c["Hkv"])
    assert lib.fasn_fwd_kvvarlen_workspace_bytes(va) == table + (blocks * nsplit * 128 * (c["D"] + 2) * 4 if nsplit > 1 else 0)
    # other offsets and lengths (other device pointers), the rows appended or not: the same launches, the same workspace
    other = _args(pkg, cu=DUMMY + 64, seqlens=DUMMY + 4096, **c)
    other.pf.kv.seqlen_add = c["Sq"]
    assert pkg._lib.kvvarlen_plan(other) == plan
    # the padded call's grid for the same step, for the record: B * Hkv * ceil(Sq / PB) blocks against items_max * Hkv
    padded = pkg._lib.kvprefill_plan(ka._args_prefill(pkg, **{k: v for k, v in c.items() if k != "T"}))
    assert padded[0][1] >= plan[1][1] // nsplit


@pytest.mark.parametrize("D", [32, 64, 128, 256])
def test_new_kernels_do_not_spill(pkg, D):
    import spill_map
    lib = os.path.join(ROOT, "flash-attention-softmax-n_amd", "libfasn.so")
    if not os.path.exists(spill_map.READELF):
        pytest.skip("llvm-readelf not available")
    table = spill_map.kernel_table(lib)
    names = sorted(table)
    pretty = subprocess.run([spill_map.CXXFILT], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    by_pretty = dict(zip(pretty, names))
    for dtype in (0, 1):
        wanted = [k[0] for k in pkg._lib.kvvarlen_plan(_args(pkg, dtype=dtype, **plan_cases()[f"D{D}_G8_small"]))] + [f"fasn_kvvarlen_append_kernel<{D}>"]
        assert len(wanted) == 4
        for name in wanted:
            hit = [m for d, m in by_pretty.items() if d.startswith("void fasn::" + name + "(")]
            assert len(hit) == 1, (name, hit)
            v = table[hit[0]]
            assert v.get("spill", 0) == 0 and v.get("scratch", 0) == 0, (name, v)


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit(__doc__)
    sys.path.insert(0, ROOT)
    import flash_attention_softmax_n_amd
    for path, text in ((MATRIX, matrix(flash_attention_softmax_n_amd)), (PLANS, plan_lines(flash_attention_softmax_n_amd))):
        with open(path, "w") as fh:
            fh.write("\n".join(text) + "\n")
        print(f"recorded {len(text)} lines in {path}")
