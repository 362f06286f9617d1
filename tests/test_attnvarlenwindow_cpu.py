"""fasn_fwd_varlen_window / fasn_bwd_varlen_window / fasn_varlen_window_plan and flash_attention_n_varlen(window=) without a GPU
(DESIGN 4.26): the codes and their order, the recorded plans (tests/golden/attn_varlen_window_plans.txt), the large window that is the
causal call, the front end's refusals, and the test of the tests - the integer model of the three walks in tests/attn_varlen_window.py
against the band mask and against the memory contract of include/fasn.h. Nothing is ever launched: the pointers are fake.

    python tests/test_attnvarlenwindow_cpu.py --record     rewrites the fixture from the library of this tree
"""
import ctypes
import inspect
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import attn_varlen as av            # noqa: E402
import attn_varlen_window as avn    # noqa: E402
import test_attnvarlen_cpu as base  # noqa: E402

PLANS = os.path.join(ROOT, "tests", "golden", "attn_varlen_window_plans.txt")
OK, EINVAL, EUNSUPPORTED = 0, -1, -7
BASE = dict(causal=True, **base.BASE)


def _codes(pkg, a, vl, win):
    """(forward, backward, forward plan, backward plan) codes through the three *_window entry points"""
    lib = pkg._lib.load()
    buf = ctypes.create_string_buffer(4096)
    return (lib.fasn_fwd_varlen_window(a.fwd if a is not None else None, vl, win, None, 0, None), lib.fasn_bwd_varlen_window(a, vl, win, None),
            lib.fasn_varlen_window_plan(a, vl, win, 0, buf, len(buf)), lib.fasn_varlen_window_plan(a, vl, win, 1, buf, len(buf)))


# ---------------------------------------------------------------- 1. codes and check order
@pytest.mark.parametrize("name", sorted(base._mutants()))
def test_base_refusals_keep_their_codes(pkg, name):
    mutate, code = base._mutants()[name]
    a, vl = av.block(pkg, **BASE)
    mutate(a, vl)
    assert _codes(pkg, a, vl, avn.window_block(pkg, 64)) == (code,) * 4, name
    # a block that breaks a base rule and a window rule answers the base rule's code
    for bad in (None, avn.window_block(pkg, 0), avn.window_block(pkg, 64, reserved=1)):
        assert _codes(pkg, a, vl, bad) == (code,) * 4, name
    a.fwd.causal = 0
    assert _codes(pkg, a, vl, avn.window_block(pkg, 64)) == (code,) * 4, name


def test_the_windows_own_refusals(pkg):
    a, vl = av.block(pkg, **BASE)
    assert all(rc > 0 for rc in _codes(pkg, a, vl, avn.window_block(pkg, 64))[2:])
    for bad in (None, avn.window_block(pkg, 0), avn.window_block(pkg, -1), avn.window_block(pkg, 64, reserved=1)):
        assert _codes(pkg, a, vl, bad) == (EINVAL,) * 4
    a.fwd.causal = 0
    assert _codes(pkg, a, vl, avn.window_block(pkg, 64)) == (EUNSUPPORTED,) * 4
    assert _codes(pkg, a, vl, avn.window_block(pkg, 1 << 30)) == (EUNSUPPORTED,) * 4   # (also where the window is the causal call)
    assert _codes(pkg, a, vl, avn.window_block(pkg, 0)) == (EINVAL,) * 4                # the operand's own rules first
    # the backward's own operands are base rules too: checked in front of the window
    lib = pkg._lib.load()
    b, vl2 = av.block(pkg, **BASE)
    b.delta = None
    assert lib.fasn_bwd_varlen_window(b, vl2, None, None) == EINVAL
    b, vl2 = av.block(pkg, **BASE)
    b.dbias.ptr = av.DUMMY
    assert lib.fasn_bwd_varlen_window(b, vl2, avn.window_block(pkg, 0), None) == EUNSUPPORTED
    buf = ctypes.create_string_buffer(4096)
    a, vl = av.block(pkg, **BASE)
    win = avn.window_block(pkg, 64)
    assert lib.fasn_varlen_window_plan(None, vl, win, 0, buf, len(buf)) == EINVAL and lib.fasn_varlen_window_plan(a, None, win, 0, buf, len(buf)) == EINVAL
    assert lib.fasn_varlen_window_plan(a, vl, win, 2, buf, len(buf)) == EINVAL and lib.fasn_varlen_window_plan(a, vl, win, 1, buf, 8) == EINVAL


# ---------------------------------------------------------------- 2. plans
def _plan_text(pkg):
    lines = []
    for name, (kw, window, which) in sorted(avn.plan_cases().items()):
        a, vl = av.block(pkg, **kw)
        lines += [f"{name} {k} grid={g} block={b} lds={l}" for k, g, b, l in pkg._lib.varlen_window_plan(a, vl, avn.window_block(pkg, window), which)]
    return lines


def test_plans_are_pinned(pkg):
    assert _plan_text(pkg) == open(PLANS).read().splitlines()


def test_plans_name_windowed_kernels_on_the_base_grids(pkg):
    """forward: tail + one forward kernel; backward: tail + dQ + dK/dV; every attention kernel a windowed packed instantiation under a name
    that is not the causal packed one; the grids those of fasn_varlen_plan on the same block"""
    seen = set()
    for name, (kw, window, which) in avn.plan_cases().items():
        a, vl = av.block(pkg, **kw)
        got = pkg._lib.varlen_window_plan(a, vl, avn.window_block(pkg, window), which)
        plain = pkg._lib.varlen_plan(a, vl, which)
        ks = [k for k, *_ in got]
        want = ["fasn_varlen_tail_kernel", "fasn_bwd_dq_kernel", "fasn_bwd_dkdv_kernel"] if which else ["fasn_varlen_tail_kernel", "fasn_fwd_kernel"]
        assert [k.split("<")[0] for k in ks] == want, name
        assert all("_varlen_window_tag" in k for k in ks[1:]), name
        assert got[0] == plain[0], name
        for (k, *rest), (k0, *rest0) in zip(got[1:], plain[1:]):
            assert k != k0 and k == k0.replace("_varlen_tag", "_varlen_window_tag") and rest == rest0, name
        seen |= {(which, window, kw["Hkv"])}
    assert {(w, win, hkv) for w in (0, 1) for win in (1, 64, 128) for hkv in (8, 2)} <= seen


# ---------------------------------------------------------------- 3. a large window is the causal call
@pytest.mark.parametrize("which", [0, 1])
def test_large_window_takes_the_causal_launches(pkg, which):
    a, vl = av.block(pkg, **{**BASE, "max_q": 300})
    assert vl.max_seqlen_k == 300
    causal = pkg._lib.varlen_plan(a, vl, which)
    for window in (300, 301, 2 ** 31 - 1):
        assert pkg._lib.varlen_window_plan(a, vl, avn.window_block(pkg, window), which) == causal, window
    assert pkg._lib.varlen_window_plan(a, vl, avn.window_block(pkg, 299), which) != causal
    lib = pkg._lib.load()
    b1, b2 = ctypes.create_string_buffer(4096), ctypes.create_string_buffer(4096)
    assert lib.fasn_varlen_plan(a, vl, which, b1, len(b1)) == lib.fasn_varlen_window_plan(a, vl, avn.window_block(pkg, 300), which, b2, len(b2)) > 0
    assert b1.value == b2.value   # the text itself


# ---------------------------------------------------------------- 4. plan independence
def test_plan_text_is_independent_of_the_pointers_and_the_token_rows(pkg):
    win = avn.window_block(pkg, 64)
    for which in (0, 1):
        a, vl = av.block(pkg, **BASE)
        b, vl2 = av.block(pkg, base=(av.DUMMY << 8) + 4096, q_token_stride=BASE["Hq"] * 64, **BASE)
        assert pkg._lib.varlen_window_plan(a, vl, win, which) == pkg._lib.varlen_window_plan(b, vl2, win, which)
        c, vl3 = av.block(pkg, q_token_stride=(BASE["Hq"] + 2 * BASE["Hkv"]) * 64, **BASE)   # q as a slice of a packed QKV buffer
        assert pkg._lib.varlen_window_plan(a, vl, win, which) == pkg._lib.varlen_window_plan(c, vl3, win, which)
        # the token rows move the tail kernel's grid alone
        d, vl4 = av.block(pkg, **{**BASE, "Tq": 4096, "Tk": 8192})
        assert pkg._lib.varlen_window_plan(a, vl, win, which)[1:] == pkg._lib.varlen_window_plan(d, vl4, win, which)[1:]


# ---------------------------------------------------------------- 5. the front end without a device
def test_front_end_refusals_without_a_device(pkg):
    fa = pkg.flash_attention_n_varlen
    q = torch.zeros(16, 4, 64, dtype=torch.bfloat16)
    cu = torch.tensor([0, 7, 16], dtype=torch.int32)
    for bad in (True, False, 64.0, torch.tensor(64), "64"):
        with pytest.raises(TypeError, match="window"):
            fa(q, q, q, cu, 9, is_causal=True, window=bad)
    for bad in (0, -1):
        with pytest.raises(ValueError, match="window must be >= 1"):
            fa(q, q, q, cu, 9, is_causal=True, window=bad)
    with pytest.raises(ValueError, match="causal and bottom-right aligned"):
        fa(q, q, q, cu, 9, window=64)
    with pytest.raises(ValueError, match="causal and bottom-right aligned"):
        fa(q, q, q, cu, 9, is_causal=False, window=64)
    with pytest.raises(RuntimeError, match="CPU tensor"):   # a legal window: the call goes on to the checks it always had
        fa(q, q, q, cu, 9, is_causal=True, window=64)


def test_signature_is_a_superset_of_todays(pkg):
    today = ["query", "key", "value", "cu_seqlens_q", "max_seqlen_q", "cu_seqlens_k", "max_seqlen_k", "softmax_n_param", "scale", "is_causal",
             "return_lse"]
    sig = inspect.signature(pkg.flash_attention_n_varlen)
    names = list(sig.parameters)
    assert names[:len(today)] == today and names[len(today):] == ["window"]
    assert sig.parameters["window"].default is None


def test_exports_and_header_agree(pkg):
    text = open(os.path.join(ROOT, "include", "fasn.h")).read()
    for name in ("fasn_fwd_varlen_window", "fasn_bwd_varlen_window", "fasn_varlen_window_plan"):
        assert name in pkg._lib.EXPORTS and f"int {name}(" in text and hasattr(pkg._lib.load(), name)
    assert "#define FASN_ABI_VERSION 6" in text and pkg._lib.load().fasn_abi_version() == 6


# ---------------------------------------------------------------- 6. the visibility model against the mask
def _sequences():
    out = []
    for name, pack in avn.PACKS.items():
        out += [(name, b, pack.lens_q[b], pack.lens_k[b]) for b in range(pack.B)]
    return out


@pytest.mark.parametrize("window", avn.WINDOWS)
def test_every_visible_element_lies_inside_the_walked_tiles(window):
    """every block of SEAMS, UNEQUAL and LONGW: every visible (i, j) of the band lies in a tile the row's wave (forward, dQ) and the key's
    wave (dK/dV) computes on, and the walked ranges keep the bounds of the memory contract"""
    starts = []
    for name, b, sq, sk in _sequences():
        m = avn.band(sq, sk, window)
        # forward and dQ: per 128-row block
        for q0 in range(0, sq, avn.BLOCK):
            w = avn.fwd_walk(sq, sk, window, q0)
            starts.append(w["klo"])
            first = avn.contract_first_key(sq, sk, window, q0)
            assert w["klo"] == first and (w["tiles"] is None or w["tiles"][0] * 64 >= first), (name, b, q0)
            for wave, tiles in enumerate(w["waves"]):
                rows = m[q0 + 32 * wave:min(q0 + 32 * wave + 32, sq)]
                cols = rows.any(0).nonzero().flatten()
                assert all(int(j) // 64 in tiles for j in cols), (name, b, q0, wave)
                if w["tiles"] is not None:
                    assert all(w["tiles"][0] <= t <= w["tiles"][1] for t in tiles)
            # a block whose rows see a key walks nothing below the tile of the first visible key
            blk = m[q0:q0 + avn.BLOCK].any(0).nonzero().flatten()
            if len(blk):
                assert w["tiles"] is not None and w["tiles"][0] == int(blk[0]) // 64 and w["tiles"][1] == int(blk[-1]) // 64, (name, b, q0)
        # dK/dV: per 128-key block
        for k0 in range(0, sk, avn.BLOCK):
            w = avn.dkdv_walk(sq, sk, window, k0)
            last = avn.contract_last_qtile(sq, sk, window, k0)
            assert w["tiles"] is None or w["tiles"][1] <= last, (name, b, k0)
            for wave, tiles in enumerate(w["waves"]):
                cols = m[:, k0 + 32 * wave:min(k0 + 32 * wave + 32, sk)]
                rows = cols.any(1).nonzero().flatten()
                assert all(int(i) // 64 in tiles for i in rows), (name, b, k0, wave)
            blk = m[:, k0:k0 + avn.BLOCK].any(1).nonzero().flatten()
            if len(blk):
                assert w["tiles"] == (int(blk[0]) // 64, int(blk[-1]) // 64), (name, b, k0)
            else:   # a key block that no row sees walks no tile
                assert w["tiles"] is None, (name, b, k0)
    if window == 64:   # LONGW is in the set for this: a rebased walk that starts two tiles and more up
        assert avn.fwd_walk(700, 700, 64, 512)["klo"] == 448 and max(starts) >= 128


def test_count_is_the_clamped_window():
    for name, b, sq, sk in _sequences():
        for window in avn.WINDOWS:
            p = torch.arange(sq) + (sk - sq)
            assert torch.equal(avn.count(sq, sk, window), torch.clamp(torch.minimum(torch.tensor(window), p + 1), min=0))


# ---------------------------------------------------------------- 7. the poison tests' premises
def test_poison_shapes_satisfy_their_premises():
    pack, window, poisoned = avn.POISON_K
    sq, sk = pack.lens_q[0], pack.lens_k[0]
    first_needed = int(avn.band(sq, sk, window).any(0).nonzero()[0])
    assert first_needed == 773 and poisoned == 64 * (first_needed // 64) == 768
    lo, hi = avn.rows_read_fwd(sq, sk, window)
    assert lo >= poisoned, "a walked K / V tile touches a poisoned row"
    for k0 in range(0, sk, avn.BLOCK):   # the key blocks wholly inside the poisoned rows walk nothing: dk / dv exactly 0
        if k0 + avn.BLOCK <= poisoned:
            assert avn.dkdv_walk(sq, sk, window, k0)["tiles"] is None
    pack, window, poisoned, judged = avn.POISON_Q
    sq = sk = pack.lens_q[0]
    reach = {k0: avn.dkdv_walk(sq, sk, window, k0)["tiles"][1] * 64 + 63 for k0 in range(0, judged, avn.BLOCK)}
    assert reach == {0: 191, 128: 319} and max(reach.values()) < poisoned
    # and what those rows' lse / delta were computed from: the forward and dQ blocks of rows below the poison read no poisoned q row
    assert max(reach.values()) < poisoned - poisoned % avn.BLOCK


if __name__ == "__main__" and "--record" in sys.argv:
    sys.path.insert(0, ROOT)
    import flash_attention_softmax_n_amd as _pkg
    open(PLANS, "w").write("\n".join(_plan_text(_pkg)) + "\n")
    print("recorded", PLANS)
