#!/usr/bin/env python3
"""Launch tables of a build of libfasn.so over a grid of calls, without a GPU:  tools/plan_sweep.py [REPO_ROOT] [OUT.txt]
(tools/plan_sweep.py [REPO_ROOT] --witness lists instead the flash_attention_n kernels that no witness plan file under tests/golden names.)
One block per call: fasn_fwd_path, fasn_bwd_path, fasn_fwd_workspace_bytes and the fasn_launch_plan text of the forward, the forward with its
workspace and the backward (dummy aligned addresses, as tests/baseline_plans.py; nothing is launched). Two trees launch the same kernels with
the same grids iff their outputs are byte-identical - run it with REPO_ROOT = an export of the other commit, built. Also lists the kernels of
the library's attention families that no plan named: an instantiation no call can reach, or an axis this sweep lacks.
The token-packed sliding-window and rotary K/V-cache calls (fasn_kvvarlen_window_plan, fasn_kvvarlen_rope_append_plan) are swept too, where the
library has them: every head dim and dtype, one split and several, with and without new rows; their kernels count as families that must be reached.
So is the shared-prefix decode (fasn_shared_prefix_plan) and its three kernels, and the prefix-groups decode (fasn_prefix_groups_plan)
and its four."""
import ctypes, hashlib, itertools, os, re, sys

ARGV = [a for a in sys.argv[1:] if not a.startswith("--")]
ROOT = os.path.abspath(ARGV[0]) if ARGV else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = ARGV[1] if len(ARGV) > 1 else None
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))]
import flash_attention_softmax_n_amd as pkg
import baseline_plans
import spill_map

L = pkg._lib
lib = L.load()
DUMMY = baseline_plans.DUMMY

# kernels of the attention families that no plan of this sweep names and that stay in the library: name -> why
KEPT_UNNAMED = {}
for _tag in ("fasn::bf16_tag", "fasn::f16_tag"):
    # launch_bwd_mode (fasn_bwd_launch.h) takes the dropout bias + key-padding instantiation of D = 128 with one query head per K/V head only; launch_bwd_one
    # compiles the grouped-K/V side (one-wave dQ, one-wave grouped dK/dV) for every dropout instantiation of a two-wave mode - no template argument tells them apart
    KEPT_UNNAMED[f"fasn_bwd_dq_kernel<{_tag}, 128, 1, 7, 1, 1, 2, 0>"] = "D = 128 dropout bias + key padding is launched with kvg == 1 only (launch_bwd_mode); a run-time argument decides"
    KEPT_UNNAMED[f"fasn_bwd_dkdv_kernel<{_tag}, 128, 1, 7, 1, 1, 1, 1, 0>"] = "D = 128 dropout bias + key padding is launched with kvg == 1 only (launch_bwd_mode); a run-time argument decides"
    # fasn_bwd_d256.hip: kvg == 1 key padding takes the two-wave kernels when the mask has unit key stride and at most kDq256KpTiles tiles; build_fwd hands
    # MODE_KEYPAD out under tighter conditions (unit stride, kFwdKpMaxTiles), so the one-wave instantiation runs with grouped K/V only - two files to show it
    KEPT_UNNAMED[f"fasn_bwd_dkdv_kernel<{_tag}, 256, 1, 6, 1, 0, 0, 2, 0>"] = "D = 256 key padding with kvg == 1 always fits the two-wave kernels; shown by build_fwd's conditions, not by a template argument"
    # fasn_fwd_d64.hip: launch_fwd_drop<Tag, 64, 2, 2> is called for plain / key-padding launches only but compiles every mode at its tuning point
    KEPT_UNNAMED[f"fasn_fwd_kernel<{_tag}, 64, 2, 1, 2, 4, 0, 1, 2, 0, 2, 1, 0, 0>"] = "launch_fwd_drop compiles all modes per tuning point; the 64-row point of D = 64 is called for plain / key padding only"

OPS = [(), ("causal",), ("keypad",), ("dense",), ("bias",), ("bias32",), ("bias", "keypad"), ("bias", "dense"), ("bias32", "keypad"), ("bias32", "dense"),
       ("causal", "bias"), ("causal", "bias32"), ("causal", "keypad"), ("causal", "dense"), ("causal", "bias", "keypad"), ("causal", "bias", "dense"), ("unaligned",)]
SHAPES = [(2, 2, 128, 128), (8, 16, 512, 512), (8, 16, 1024, 1024), (4, 16, 1536, 1536), (4, 16, 2048, 2048), (8, 16, 4096, 4096), (4, 32, 8192, 8192),
          (64, 16, 4096, 4096), (1, 16, 1, 16384), (1, 16, 128, 16384), (4, 16, 1024, 4096),
          (1, 4, 256, 33792)]   # (more key tiles than the key-padding table holds)


def view(v, strides, ptr=DUMMY):
    v.ptr = ptr
    for i, s in enumerate(strides):
        v.stride[i] = s


def make_args(B, H, Sq, Sk, D, dt, ops, drop, g, dbias, scale):
    a = L.BwdArgs()
    f = a.fwd
    Hk = H // g
    for v in (f.q, f.o, a.dout, a.dq):
        view(v, (H * Sq * D, Sq * D, D, 1))
    for v in (f.k, f.v, a.dk, a.dv):
        view(v, (Hk * Sk * D, Sk * D, D, 1))
    f.lse = DUMMY
    a.delta = DUMMY
    f.dtype, f.B, f.H, f.Sq, f.Sk, f.D, f.Dv = dt, B, H, Sq, Sk, D, D
    f.scale = scale if scale is not None else 1.0 / D ** 0.5
    f.softmax_n, f.causal, f.dropout_p, f.kv_group = 1.0, int("causal" in ops), drop, (g if g > 1 else 0)
    if "keypad" in ops:
        view(f.mask, (Sk, 0, 0, 1))
    if "dense" in ops:
        view(f.mask, (H * Sq * Sk, Sq * Sk, Sk, 1))
    if "unaligned" in ops:   # a dense mask whose rows do not move as 4-byte vectors
        view(f.mask, (H * Sq * (Sk + 1), Sq * (Sk + 1), Sk + 1, 1), ptr=DUMMY + 1)
    if "bias" in ops or "bias32" in ops:
        view(f.bias, (0, Sq * Sk, Sk, 1))
        f.bias_dtype = L.FASN_BIAS_F32 if "bias32" in ops else L.FASN_BIAS_SAME
        if dbias == "dense":
            view(a.dbias, (H * Sq * Sk, Sq * Sk, Sk, 1))
        if dbias == "reduced":
            view(a.dbias, (0, Sq * Sk, Sk, 1))
            a.dbias_dtype = f.bias_dtype
    return a


def calls():
    for D, dt, ops, drop, g, (B, H, Sq, Sk) in itertools.product((32, 64, 128, 256), (0, 1, 2), OPS, (0.0, 0.1), (1, 4), SHAPES):
        has_bias = any(o.startswith("bias") for o in ops)
        for dbias in ((None, "dense", "reduced") if has_bias else (None,)):
            for scale in ((None, 40.0) if (dt == 0 and (B, H, Sq) == (8, 16, 1024)) else (None,)):   # fp16 with |scale * log2e| > 8: element loads
                yield (f"D={D} dt={dt} ops={'+'.join(ops) or 'none'} p={drop} g={g} {B}x{H}x{Sq}x{Sk} dbias={dbias} scale={scale}",
                       make_args(B, H, Sq, Sk, D, dt, ops, drop, g, dbias, scale))
    for name in baseline_plans.CONFIGS:
        yield f"baseline {name}", baseline_plans.bwd_args(pkg, name)


def kv_packed_calls():
    """(header, plan function, its operands) of the packed window and rotary calls: fasn_kvvarlen_args over dummy addresses, q / o / q_out /
    k_new / v_new as [1, heads, T, D] views of [T, heads, D] buffers"""
    if not hasattr(lib, "fasn_kvvarlen_window_plan"):   # (a tree from before these calls)
        return
    for D, dt, (H, Hkv), (B, Sq, T, pages) in itertools.product((32, 64, 128, 256), (0, 1), ((8, 8), (64, 8), (12, 4)),
                                                                ((4, 48, 64, 64), (257, 4096, 4352, 32), (3, 40, 51, 16))):
        def block(add):
            va = L.KvVarlenArgs()
            a = va.pf.kv
            for v in (a.q, a.o):
                view(v, (0, D, H * D, 1))
            a.lse = a.k_cache = a.v_cache = a.block_table = a.seqlens = DUMMY
            for i, st in enumerate((256 * Hkv * D, Hkv * D, D)):
                a.k_stride[i] = a.v_stride[i] = st
            a.block_table_stride = a.max_pages = pages
            a.seqlen_add, a.page_size = (Sq if add else 0), 256
            a.B, a.H, a.kv_group, a.Sq, a.D, a.dtype = B, H, H // Hkv, Sq, D, dt
            a.scale, a.softmax_n, a.causal = D ** -0.5, 1.0, 1
            va.cu_seqlens_q, va.total_tokens, va.reserved = DUMMY, T, 0
            return va
        hdr = f"kvvarlen D={D} dt={dt} heads={H}/{Hkv} B={B} Sq={Sq} T={T} pages={pages}"
        for W in (1, 128, 3000, 2 ** 31 - 1):
            yield f"{hdr} window={W}", lib.fasn_kvvarlen_window_plan, (block(False), L.KvWindow(window=W, reserved=0))
        rope = L.KvRope()
        rope.cos = rope.sin = DUMMY
        rope.row_stride, rope.rows, rope.rotary_dim, rope.table_dtype, rope.interleaved = D // 2, 256 * pages, D, L.FASN_DTYPE_F32, 0
        qo, kn = L.View4(), L.View4()
        view(qo, (0, D, H * D, 1))
        view(kn, (0, D, Hkv * D, 1))
        yield f"{hdr} rope+append", lib.fasn_kvvarlen_rope_append_plan, (block(True), rope, qo, kn, kn)
        yield f"{hdr} rope", lib.fasn_kvvarlen_rope_append_plan, (block(False), rope, qo, None, None)


def shared_prefix_calls():
    """(header, plan function, its operands) of the shared-prefix decode: a fasn_kvcache_args over dummy addresses and the prefix operand -
    both head dims and dtypes, one row block and several, a prefix of one split and of several"""
    if not hasattr(lib, "fasn_shared_prefix_plan"):   # (a tree from before this call)
        return
    for D, dt, (H, Hkv), (B, Sq, pages, ppages) in itertools.product((64, 128), (0, 1), ((8, 8), (64, 8), (6, 2)),
                                                                    ((64, 1, 40, 32), (1, 1, 40, 32), (10, 5, 8, 3), (4, 16, 32, 48))):
        a = L.KvCacheArgs()
        for v in (a.q, a.o):
            view(v, (H * Sq * D, Sq * D, D, 1))
        a.lse = a.k_cache = a.v_cache = a.block_table = a.seqlens = DUMMY
        for i, st in enumerate((256 * Hkv * D, Hkv * D, D)):
            a.k_stride[i] = a.v_stride[i] = st
        a.block_table_stride = a.max_pages = pages
        a.seqlen_add, a.page_size = 0, 256
        a.B, a.H, a.kv_group, a.Sq, a.D, a.dtype = B, H, H // Hkv, Sq, D, dt
        a.scale, a.softmax_n, a.causal = D ** -0.5, 1.0, 1
        yield (f"shared_prefix D={D} dt={dt} heads={H}/{Hkv} B={B} Sq={Sq} pages={pages} prefix_pages={ppages}", lib.fasn_shared_prefix_plan,
               (a, L.SharedPrefix(prefix_len=DUMMY, prefix_table=DUMMY, max_prefix_pages=ppages, reserved=0)))


def prefix_groups_calls():
    """the blocks of shared_prefix_calls() behind 1, 4 and 64 prefix groups (fasn_prefix_groups_plan)"""
    if not hasattr(lib, "fasn_prefix_groups_plan"):   # (a tree from before this call)
        return
    for hdr, _plan, (a, sp) in shared_prefix_calls():
        for G in (1, 4, 64):
            yield (hdr.replace("shared_prefix", "prefix_groups") + f" groups={G}", lib.fasn_prefix_groups_plan,
                   (a, L.PrefixGroups(prefix_lens=DUMMY, prefix_tables=DUMMY, prefix_group=DUMMY, num_groups=G,
                                      max_prefix_pages=sp.max_prefix_pages, reserved=0)))


def library_attention_kernels():
    table = spill_map.kernel_table(os.path.join(ROOT, "flash-attention-softmax-n_amd", "libfasn.so"))
    names = {re.sub(r"\(fasn::\w+(, fasn::\w+)*\)$", "", d).replace("void fasn::", "") for d in spill_map.demangle(list(table)).values()}
    return names, {n for n in names if re.match(r"fasn_(fwd|bwd|f32)_|fasn_kvvarlen_(fwd_window|rope)_kernel|fasn_kvshared_|fasn_kvgroups_", n)}


def witness_main():
    """tools/plan_sweep.py [REPO_ROOT] --witness: the flash_attention_n kernels of the library (fasn_fwd_ / fasn_bwd_ / fasn_f32_) that no
    witness plan file under tests/golden names (attn_witness_plans.txt, bias_witness_plans.txt and their siblings) - what the witnesses
    do not reach. No sweep is run."""
    gold = os.path.join(ROOT, "tests", "golden")
    named = set()
    files = sorted(f for f in os.listdir(gold) if f.endswith("witness_plans.txt"))
    for f in files:
        for line in open(os.path.join(gold, f)):
            if line.startswith("    fasn_"):
                named.add(line.strip().split(" grid=")[0])
    _, att = library_attention_kernels()
    att = {n for n in att if re.match(r"fasn_(fwd|bwd|f32)_", n)}
    miss = sorted(att - named)
    print(f"witness plan files {', '.join(files)}: {len(att & named)} of {len(att)} flash_attention_n kernels named, {len(miss)} not")
    for n in miss:
        print("   ", n)
    return 0


def main():
    if "--witness" in sys.argv:
        return witness_main()
    out, named, ncalls = [], set(), 0
    buf = ctypes.create_string_buffer(1 << 15)
    for hdr, plan, operands in itertools.chain(kv_packed_calls(), shared_prefix_calls(), prefix_groups_calls()):
        ncalls += 1
        rc = plan(*operands, buf, len(buf))
        out.append(f"{hdr} rc={rc}")
        for line in buf.value.decode().splitlines():
            out.append("    " + line)
            named.add(line.split(" grid=")[0])
    for hdr, a in calls():
        ncalls += 1
        out.append(f"{hdr} fwd_path={lib.fasn_fwd_path(a.fwd)} bwd_path={lib.fasn_bwd_path(a)} ws={lib.fasn_fwd_workspace_bytes(a.fwd)}")
        for which in (L.FASN_PLAN_FWD, L.FASN_PLAN_FWD_WS, L.FASN_PLAN_BWD):
            rc = lib.fasn_launch_plan(a, which, buf, len(buf))
            out.append(f"  [{which}] rc={rc}")
            for line in buf.value.decode().splitlines():
                out.append("    " + line)
                named.add(line.split(" grid=")[0])
    text = "\n".join(out) + "\n"
    if OUT:
        open(OUT, "w").write(text)
    print(f"{ncalls} calls, {len(out)} lines, sha256 {hashlib.sha256(text.encode()).hexdigest()}")
    names, att = library_attention_kernels()
    miss = sorted(att - named)
    print(f"library kernels {len(names)}, attention families {len(att)}, named by the sweep {len(att & named)}, named but not in the library {len(named - names)}, never named {len(miss)}")
    for n in miss:
        print("   ", n, "--", KEPT_UNNAMED.get(n, "NO REASON GIVEN"))
    return 1 if (named - names) or any(n not in KEPT_UNNAMED for n in miss) else 0


if __name__ == "__main__":
    sys.exit(main())
