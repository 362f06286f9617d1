"""What the FP8 token-tree tests share (tests/test_kvfp8_tree_cpu.py, tests/test_gpu_kvfp8_tree.py): the cases of the bit-for-bit comparison
with the 16-bit tree call and their operands - built the same way on the CPU and on the GPU, so that the CPU suite can check from the fp32
reference alone that a case leaves the exact comparison enough normal numbers - the mask rows, the poisoning below a tree's window and the
fp32 reference on the dequantised cache. Built on tests/kv_fp8.py and tests/kv_tree.py, which stay as they are. A plain module: no tests,
importable without a GPU."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_fp8 as k8       # noqa: E402
import kv_support as ks   # noqa: E402
import kv_tree as kt      # noqa: E402


def rows_of(kind, Sq, B, seed):
    """[B][Sq] words: "chain", "tree" (random parents), "star", "arbitrary" (any 64-bit words) or "self" (a node sees itself alone)"""
    gen = torch.Generator().manual_seed(seed)
    make = {"chain": lambda: kt.chain(Sq), "tree": lambda: kt.random_tree(Sq, gen)[0], "star": lambda: kt.star(Sq),
            "arbitrary": lambda: kt.arbitrary(Sq, gen), "self": lambda: [1 << i for i in range(Sq)]}[kind]
    return [make() for _ in range(B)]


def route_of(H, Hkv, Sq, qlens):
    return "decode" if qlens is None and (H // Hkv) * Sq <= 128 else "prefill"


# The cases of "equal to the 16-bit tree call, bit for bit". `prefix`: base_b; the nodes are cache rows already (len_b = base_b + qlen_b).
# decode / prefill: the nodes straddle a tile edge (56), start on one (64) or are the whole cache (0). full: bit 63 is an ordinary bit, on
# the decode kernels at 128 rows (G = 2) and on the prefill kernels (G = 4). split: plans with more than one split (asserted from the plan).
# window: W = 70 with whole pages below first_b = 64 floor(max(0, base_b - 69) / 64) - 128 rows at base 200, 64 at base 135.
TWIN_CASES = {
    "decode_tree": dict(H=8, Hkv=2, Sq=16, page=64, max_pages=4, prefix=[56, 64, 0], kind="tree", seed=301),
    "decode_arbitrary": dict(H=8, Hkv=2, Sq=16, page=64, max_pages=4, prefix=[56, 64, 0], kind="arbitrary", seed=302),
    "prefill_tree": dict(H=8, Hkv=2, Sq=40, page=64, max_pages=4, prefix=[56, 64, 0], qlens=[40, 7, 0], kind="tree", seed=303),
    "prefill_arbitrary": dict(H=8, Hkv=2, Sq=40, page=64, max_pages=4, prefix=[56, 64, 0], qlens=[40, 7, 0], kind="arbitrary", seed=304),
    "full_g2": dict(H=4, Hkv=2, Sq=64, page=64, max_pages=4, prefix=[0, 61], kind="arbitrary", seed=305),
    "full_g4": dict(H=8, Hkv=2, Sq=64, page=64, max_pages=4, prefix=[0, 61], kind="arbitrary", seed=306),
    "split_decode": dict(H=2, Hkv=1, Sq=16, page=64, max_pages=64, prefix=[3000], kind="tree", seed=307, splits=True),
    "split_prefill": dict(H=2, Hkv=1, Sq=16, page=64, max_pages=64, prefix=[3000], qlens=[13], kind="arbitrary", seed=308, splits=True),
    "window_decode_tree": dict(H=8, Hkv=2, Sq=16, page=64, max_pages=4, prefix=[200, 135, 0], kind="tree", seed=309, window=70),
    "window_decode_arbitrary": dict(H=8, Hkv=2, Sq=16, page=64, max_pages=4, prefix=[200, 135, 0], kind="arbitrary", seed=310, window=70),
    "window_prefill_tree": dict(H=8, Hkv=2, Sq=40, page=64, max_pages=4, prefix=[200, 135, 0], qlens=[40, 7, 0], kind="tree", seed=311, window=70),
    "window_prefill_arbitrary": dict(H=8, Hkv=2, Sq=40, page=64, max_pages=4, prefix=[200, 135, 0], qlens=[40, 7, 0], kind="arbitrary", seed=312,
                                     window=70),
}


def twin_operands(case, D, dtype, dev):
    """the operands of one TWIN_CASES entry: counter-based or CPU-generated, so identical on every device"""
    c = TWIN_CASES[case]
    B, H, Hkv, Sq, seed = len(c["prefix"]), c["H"], c["Hkv"], c["Sq"], c["seed"]
    ql = list(c.get("qlens") or [Sq] * B)
    lens = [p + x for p, x in zip(c["prefix"], ql)]
    Smax = c["page"] * c["max_pages"]
    assert max(lens) <= Smax
    return dict(B=B, H=H, Hkv=Hkv, Sq=Sq, D=D, page=c["page"], max_pages=c["max_pages"], Smax=Smax, qlens=c.get("qlens"), ql=ql, lens=lens,
                window=c.get("window"), rows=rows_of(c["kind"], Sq, B, seed), q=ks._rand((B, H, Sq, D), dtype, dev, seed + 10),
                kd=k8.rand_codes((B, Hkv, Smax, D), seed + 11, dev), vd=k8.rand_codes((B, Hkv, Smax, D), seed + 12, dev),
                k_scale=k8.scales_bh(k8.POW2_SCALES, B, Hkv, dev, seed + 13), v_scale=k8.scales_bh(k8.POW2_SCALES, B, Hkv, dev, seed + 14),
                n=ks._n_values((B, H), dev, seed + 15))


def reference_fp8_tree(q, kd, vd, lens, ql, n, masks, k_scale, v_scale, window=None, scale=None, dequantise_v=True):
    """kv_tree.reference_tree (fp32) on the dequantised visible cache: up(code) * scale[b, hkv]. dequantise_v=False leaves V as up(code) -
    the 16-bit twin's own out, which v_scale multiplies afterwards"""
    kg = k8.up(k8.visible(kd, lens)) * k_scale[:, :, None, None]
    vg = k8.up(k8.visible(vd, lens))
    if dequantise_v:
        vg = vg * v_scale[:, :, None, None]
    return kt.reference_tree(q, kg, vg, lens, ql, n, masks, window, scale)


def subnormal_fraction(out16, vs_h, dtype):
    """the share of elements kv_fp8.assert_bitwise leaves out of the exact comparison, from the twin's out (as fp32) and v_scale per query
    head: those where the 16-bit call's result or its product with v_scale is a subnormal number of `dtype`"""
    tiny = 2.0 ** -14 if dtype == torch.float16 else 2.0 ** -126
    want32 = out16 * vs_h[:, :, None, None]
    exact = ((out16.abs() >= tiny) & (want32.abs() >= tiny)) | (out16 == 0)
    return (~exact).float().mean().item()


def poison_below(pc, lens, ql, W):
    """every cache row below first_b = 64 * floor(max(0, base_b - W + 1) / 64), base_b = len_b - qlen_b, becomes the NaN code and the table
    entry of every page wholly below first_b names the poison page (pc: kv_fp8.PagedCodes). Returns the rows poisoned."""
    tbl = pc.table.cpu()
    rows = 0
    for b, (ln, x) in enumerate(zip(lens, ql)):
        first = ks._first(ln, x, W)
        rows += first
        for s in range(-(-first // pc.page)):
            pid, cnt = int(tbl[b, s]), min(pc.page, first - s * pc.page)
            pc.ku[pid, :cnt] = k8.NAN_CODE
            pc.vu[pid, :cnt] = k8.NAN_CODE
        pc.table[b, :first // pc.page] = pc.poison
    return rows
