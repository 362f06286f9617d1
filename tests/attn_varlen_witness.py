"""The three witnesses of tests/attn_witness.py brought to flash_attention_n_varlen: a pack is a list of rectangular
problems, and every sequence of it is judged by the fp64 reference and the gates that attn_witness.py derives - no tolerance is new here.

Why. tests/attn_varlen.py draws logits of standard deviation 0.25 and gates one number per tensor: in a 300-key sequence one key too many
at the causal limit, a bottom-right offset taken from the neighbouring sequence or an lse row of the wrong head stays below that gate
(the argument of attn_witness's docstring, unchanged). The packed kernels compute every length, base pointer, descriptor range and
lse / delta base per work item from device memory (varlen_enter_fwd, varlen_enter_bwd, varlen_head_bwd, varlen_stat), and place their
items through block_to_work / block_to_work_grouped on a grid sized from the hints.

  WPack     named packs: the lengths of both sides, H, Hkv and the tail rows. Sequence b is the attn_witness.Case(1, H, sq_b, sk_b, 64, Hkv)
            with ub = 1, uh = H; its operands come from aw.inputs_a / inputs_b / inputs_c with the pack's one n [H] handed in.
  world     operands of every sequence laid into [T, H, 64] / [T, Hkv, 64] at the pack's offsets, the rows behind cu[B] (and the rows of a
            sequence whose other side is empty) filled with finite junk; the fp64 reference and the gates per sequence; world() keeps
            the few that several tests share
  run       flash_attention_n_varlen and its backward, once
  cut       the packed results back into per-sequence dicts of the shape aw.run returns
  judge     aw.judge_a / judge_b / judge_c per sequence, every (sequence, head, row) with sq_b > 0; dn - one [H] tensor for the call - against
            the sum of the sequences' references under the sum of their gates; sequences with an empty side and the tail rows exactly
            (0, log n or -inf, gradients 0)
  model     the item maps in integers: block_to_work, causal_head_group, block_to_work_grouped (csrc/fasn_common.h) and the launch
            sizes of csrc/fasn_attnvarlen.hip

The launched kernels are the one-wave D = 64 forward, fasn_bwd_dq_kernel and fasn_bwd_dkdv_kernel: no *_ws kernel, so rounding point (7) of
witness C does not apply (Case.p_rounded is False: the cases name no plan property).

Witness A in bf16. A class of the indicator pattern holds 32 keys per half tile and 31 classes: beyond 992 keys a class holds 64, and
64 u = 0.25 > 0.2 in bf16 (attn_witness.SHAPES runs such shapes in fp16 only). The sequences of 1100 keys therefore carry witness A's
operands in bf16 too but are judged there by witness C's per-element gates (a_integer() says which); in fp16 every sequence runs under
the integer gates.

A helper module: no test is collected from it. tests/test_attnvarlenwitness_cpu.py is the test of these tests,
tests/test_gpu_attnvarlenwitness.py runs the kernels."""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_witness as aw   # noqa: E402
import attn_varlen as av    # noqa: E402

D = 64
BLOCK = 128     # query rows / keys of a work item (kBlock in csrc/fasn_attnvarlen.hip)
S_STAR = 300    # the key length at which witness A's n makes Z a power of two
N_A = float((1 << S_STAR.bit_length()) - S_STAR)   # 212


class WPack:
    def __init__(self, name, lens_q, lens_k=None, H=4, Hkv=4, tail=25, T=None):
        self.name, self.H, self.Hkv = name, H, Hkv
        self.pack = av.Pack(lens_q, lens_k, tail_q=tail)
        if T is not None:   # a fixed number of token rows whatever the offsets say
            self.pack.Tq = self.pack.Tk = T
        assert H % Hkv == 0

    @property
    def key(self):
        p = self.pack
        return (self.name, tuple(p.lens_q), tuple(p.lens_k), self.H, self.Hkv, p.Tq, p.Tk)

    def case(self, b, causal, n_pos=None):
        p = self.pack
        return aw.Case(1, self.H, p.lens_q[b], p.lens_k[b], D, self.Hkv, causal=causal, ub=1, uh=self.H, n_pos=n_pos)

    def live(self):
        """the sequences with rows AND keys: the ones the witnesses judge"""
        p = self.pack
        return [b for b in range(p.B) if p.lens_q[b] > 0 and p.lens_k[b] > 0]


LONG8_Q = [1100, 0, 130, 517, 64, 1, 300, 959]
LONG8_K = [700, 64, 0, 1100, 64, 300, 300, 31]
LONG4_Q = [900, 257, 1, 640]
MANY_LENS = [(1, 2, 3, 0)[b % 4] for b in range(512)]


def long8(Hkv=4, unequal=False):
    return WPack("LONG8 unequal" if unequal else "LONG8 self", LONG8_Q, LONG8_K if unequal else None, H=4, Hkv=Hkv, tail=25)


def long4(H=8, Hkv=1):
    return WPack("LONG4", LONG4_Q, None, H=H, Hkv=Hkv, tail=25)


def many(empty_from=None):
    """512 sequences of 1, 2, 3, 0 tokens; empty_from: the offsets stay constant from that sequence on (a trailing run of empty
    sequences) while the operands keep their rows"""
    lens = list(MANY_LENS)
    T = sum(lens) + 25
    if empty_from is not None:
        lens = [x if b < empty_from else 0 for b, x in enumerate(lens)]
    return WPack("MANY" if empty_from is None else f"MANY empty from {empty_from}", lens, None, H=4, Hkv=4, T=T)


def n_of(wp, wit):
    """the call's one n [H], fp32 on the CPU. A: 0 in head 0 and N_A elsewhere (Z = N_A + 300 = 512 in the sequences of 300 keys).
    B, C: zeros next to positive entries as aw.n_values draws them - one sign per K/V head's group where there are two groups (judge_b
    gates dK / dV of a group only where the whole group is decided), per head under a single K/V head."""
    h = torch.arange(wp.H)
    if wit == "A":
        return torch.where(h == 0, 0.0, N_A).float()
    g = h // (wp.H // wp.Hkv) if wp.Hkv >= 2 else h
    return torch.where(g % 2 == 0, 0.0, 0.5 + 0.75 * g.double()).float()


def a_integer(case, dtype):
    """witness A's integer gates apply: the largest class count of aw.inputs_a's pattern times u stays at or below 0.2, the condition
    aw.condition_a asserts from the reference (module docstring). A class of the second half holds whole granules, every 31st one; a
    class of the first half every 32nd key."""
    gran, classes = aw.GRANULE[dtype], D // 2 - 1
    count = max(gran * -(-(-(-case.S // gran)) // classes), -(-case.S // (D // 2)))
    return count * aw.U[dtype] <= 0.2


# ---------------------------------------------------------------- operands, reference and gates of a pack
class World:
    """One (pack, witness, operands): per live sequence b the case, its inputs, the fp64 reference r and witness C's gates g; the packed
    operands q, k, v, do, n on `dev`. Never modified."""

    def __init__(self, wp, wit, dtype, dev, causal, form=None, std=None, seed=0, backward=True, only=None):
        self.wp, self.wit, self.dt, self.dev, self.causal, self.form, self.std, self.backward = wp, wit, dtype, dev, causal, form, std, backward
        p = wp.pack
        self.n = n_of(wp, wit)
        self.seq = {}
        g = torch.Generator().manual_seed(900 + seed)
        junk = lambda T, heads: (2.0 * torch.randn(T, heads, D, generator=g)).to(dtype).to(dev)   # noqa: E731  (finite junk: tail rows, rows facing an empty side)
        self.q, self.do = junk(p.Tq, wp.H), junk(p.Tq, wp.H)
        self.k, self.v = junk(p.Tk, wp.Hkv), junk(p.Tk, wp.Hkv)
        self.scale = None
        u, ua = aw.U[dtype], aw.unit_abs(dtype)
        for b in wp.live():
            if only is not None and b not in only:   # (the test of the tests: the sequences it mutates)
                continue
            case = wp.case(b, causal, n_pos=N_A if wit == "A" else None)
            sd = 7919 * seed + 31 * b + 5
            if wit == "A":
                inp = aw.inputs_a(case, dtype, dev, sd, n=self.n)
            elif wit == "B":
                inp = aw.inputs_b(case, form, dtype, dev, sd, n=self.n)
            else:
                inp = aw.inputs_c(case, std, dtype, dev, sd, n=self.n)
            assert self.scale in (None, inp["scale"]), "one scale per call"
            self.scale = inp["scale"]
            rq, rk = av.seq_rows(p, "q", b), av.seq_rows(p, "k", b)
            self.q[rq], self.do[rq] = inp["q"][0].transpose(0, 1), inp["do"][0].transpose(0, 1)
            self.k[rk], self.v[rk] = inp["k"][0].transpose(0, 1), inp["v"][0].transpose(0, 1)
            r = aw.reference(case, inp, backward=backward)
            gates = aw.with_bounds(case, inp, r, u, ua)
            inp = {key: (val.cpu() if torch.is_tensor(val) else val) for key, val in inp.items()}   # (the packed copies above are what stays on the device)
            self.seq[b] = (case, inp, r, gates)
        if self.scale is None:
            self.scale = 1.0 / math.sqrt(D)

    def packed(self):
        return dict(q=self.q, k=self.k, v=self.v, do=self.do, n=self.n.to(self.dev), scale=self.scale)


_WORLDS = {}


def world(wp, wit, dtype, dev, causal, form=None, std=None, seed=0, backward=True, only=None):
    """a World kept for the tests that share it (a world holds the fp64 reference and gates of every sequence, several [H, L, S]
    tensors each: what one test alone uses is built with World(...) and dropped with the test)"""
    key = (wp.key, wit, dtype, str(dev), causal, form, std, seed, backward, None if only is None else tuple(only))
    if key not in _WORLDS:
        _WORLDS[key] = World(wp, wit, dtype, dev, causal, form, std, seed, backward, only)
    return _WORLDS[key]


def forget_worlds():
    """drop the shared worlds: their references on the host and their packed operands on the device (a GPU test module calls it when
    it is done: the suite's later modules measure their own peak memory)"""
    _WORLDS.clear()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


# ---------------------------------------------------------------- the call
def run(pkg, wp, ops, causal, backward=True, hints=None, cu=None, scale=None):
    """flash_attention_n_varlen on the packed operands `ops` (World.packed()) and its backward with ops["do"]: out [Tq, H, D],
    lse [H, Tq], dq, dk, dv, dn [H] (None without a backward). hints: (max_seqlen_q, max_seqlen_k) instead of the tight ones"""
    p = wp.pack
    dev = ops["q"].device
    cu_q, cu_k = p.cu(dev) if cu is None else cu
    max_q, max_k = (p.max_q, p.max_k) if hints is None else hints
    kw = dict(cu_seqlens_k=None if p.self_attn else cu_k, max_seqlen_k=max_k, scale=ops["scale"] if scale is None else scale,
              is_causal=causal, return_lse=True)
    if not backward:
        with torch.no_grad():
            out, lse = pkg.flash_attention_n_varlen(ops["q"], ops["k"], ops["v"], cu_q, max_q, softmax_n_param=ops["n"], **kw)
        torch.cuda.synchronize(dev)
        return dict(out=out, lse=lse, dq=None, dk=None, dv=None, dn=None)
    q, k, v, n = (ops[x].detach().clone().requires_grad_() for x in ("q", "k", "v", "n"))
    out, lse = pkg.flash_attention_n_varlen(q, k, v, cu_q, max_q, softmax_n_param=n, **kw)
    out.backward(ops["do"])
    torch.cuda.synchronize(dev)
    return dict(out=out.detach(), lse=lse.detach(), dq=q.grad, dk=k.grad, dv=v.grad, dn=n.grad)


def cut(wp, raw, b):
    """sequence b of a packed result in the layout of aw.run: out, dq [1, H, sq, D], lse [1, H, sq], dk, dv [1, Hkv, sk, D] on the CPU;
    dn None (one tensor for the call: judge() gates it over the pack)"""
    p = wp.pack
    rq, rk = av.seq_rows(p, "q", b), av.seq_rows(p, "k", b)
    rows = lambda t, r: None if t is None else t[r].transpose(0, 1).unsqueeze(0).cpu()   # noqa: E731
    return dict(out=rows(raw["out"], rq), lse=raw["lse"][:, rq].unsqueeze(0).cpu(), dq=rows(raw["dq"], rq), dk=rows(raw["dk"], rk),
                dv=rows(raw["dv"], rk), dn=None, dbias=None, state=None)


def as_raw(wp, w, rs=None, dtype=None):
    """what kernels that computed exactly the references `rs` (b -> a reference() result; default: the world's own) would return for the
    pack, on the CPU: the test of the tests feeds it through cut() and judge()"""
    p = wp.pack
    dt = w.dt if dtype is None else dtype
    bwd = w.backward
    out = torch.zeros(p.Tq, wp.H, D, dtype=dt)
    lse = torch.full((wp.H, p.Tq), -math.inf)
    dq = torch.zeros(p.Tq, wp.H, D, dtype=dt) if bwd else None
    dk, dv = (torch.zeros(p.Tk, wp.Hkv, D, dtype=dt) for _ in range(2)) if bwd else (None, None)
    dn = torch.zeros(wp.H, dtype=torch.float64) if bwd else None
    n = w.n.double()
    for b in range(p.B):
        rq, rk = av.seq_rows(p, "q", b), av.seq_rows(p, "k", b)
        if b not in w.seq:
            lse[:, rq] = torch.where(n > 0, torch.log(n), torch.full_like(n, -math.inf)).float().view(-1, 1)
            continue
        case = w.seq[b][0]
        res = aw.as_result(case, (rs or {}).get(b, w.seq[b][2]), dt, backward=bwd)
        out[rq], lse[:, rq] = res["out"][0].transpose(0, 1), res["lse"][0]
        if bwd:
            dq[rq], dk[rk], dv[rk] = res["dq"][0].transpose(0, 1), res["dk"][0].transpose(0, 1), res["dv"][0].transpose(0, 1)
            dn += (rs or {}).get(b, w.seq[b][2])["dn"][0]
    return dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv, dn=None if dn is None else dn.float())


# ---------------------------------------------------------------- the gates of a pack
def judge_seq(w, b, res, rat=None, kinds=None):
    """sequence b's cut result under its witness: the ratios merged into `rat`, the row kinds of witness B into `kinds`"""
    case, inp, r, g = w.seq[b]
    rat = aw.Ratios() if rat is None else rat
    if w.wit == "A":
        if a_integer(case, w.dt):
            aw.condition_a(case, r, w.dt, 0.0)
            one = aw.judge_a(case, w.dt, res, r, g if w.backward else None)
        else:
            one = aw.judge_c(case, w.dt, res, r, g)
    elif w.wit == "B":
        one, k = aw.judge_b(case, w.form, w.dt, res, r, g, inp)
        if kinds is not None:
            kinds |= k
    else:
        one = aw.judge_c(case, w.dt, res, r, g)
    for key, val in one.items():
        rat.up(key, val)
    return rat


def gate_dn(w, dn, rat, rs=None):
    """the call's dn [H] against the sum of the sequences' references. A, C: under the sum of their gates + 1e-6 (judge_c's allowance,
    once). B (bounded code): 1e-6, in the heads every sequence decides (judge_b's rule: a head without a sink is undecided in code_sink)"""
    want, gate = torch.zeros(w.wp.H, dtype=torch.float64), torch.zeros(w.wp.H, dtype=torch.float64)
    for b, (case, inp, r, g) in w.seq.items():
        want += r["dn"][0]
        if "dn" in g:
            gate += g["dn"][0]
    if w.wit == "B":
        live = torch.ones(w.wp.H, dtype=torch.bool) if w.form != "code_sink" else (w.n > 0)
        rat.up("dn", aw.ratio(dn.cpu()[live], want[live], torch.full_like(want[live], 1e-6)))
    else:
        rat.up("dn", aw.ratio(dn.cpu(), want, gate + 1e-6))


def exact_rest(wp, w, raw, rat=None):
    """what no witness judges: a sequence without keys is exactly 0 with dq exactly 0 and lse = log n - exactly -inf at n = 0, within the
    fp32 term of witness C's lse gate, 2^-22 (1 + |log n|), elsewhere (rounding point 4: no weight is summed, no logit formed) -; the
    dk / dv rows of a sequence without queries are exactly 0; rows at or beyond cu[B]: out, dq, dk, dv 0 and lse -inf, exactly"""
    p = wp.pack
    bwd = raw.get("dq") is not None
    n = w.n.double()
    logn = torch.where(n > 0, torch.log(n), torch.full_like(n, -math.inf)).view(-1, 1)
    for b in range(p.B):
        if b in w.seq:
            continue
        rq, rk = av.seq_rows(p, "q", b), av.seq_rows(p, "k", b)
        assert (raw["out"][rq].float() == 0).all(), f"sequence {b} without keys: out not 0"
        if rq.stop > rq.start:
            got, want = aw._lse_pair(raw["lse"][:, rq].cpu(), logn.expand(-1, rq.stop - rq.start))
            one = aw._ratio((got - want).abs(), 2.0 ** -22 * (1 + want.abs()))
            if rat is not None:
                rat.up("lse (no key)", one)
            assert one <= 1, f"sequence {b} without keys: lse is not log n ({one:.3g} of 2^-22 (1 + |log n|))"
        if bwd:
            assert (raw["dq"][rq].float() == 0).all(), f"sequence {b} without keys: dq not 0"
            assert (raw["dk"][rk].float() == 0).all() and (raw["dv"][rk].float() == 0).all(), f"sequence {b} without queries: dk / dv not 0"
    eq, ek = p.cu_q[-1], p.cu_k[-1]
    assert (raw["out"][eq:].float() == 0).all() and (raw["lse"][:, eq:] == -math.inf).all(), "rows behind the last sequence: out not 0 / lse not -inf"
    if bwd:
        assert (raw["dq"][eq:].float() == 0).all(), "rows behind the last sequence: dq not 0"
        assert (raw["dk"][ek:].float() == 0).all() and (raw["dv"][ek:].float() == 0).all(), "key rows behind the last sequence: dk / dv not 0"


def judge(w, raw):
    """(ratios, row kinds) of a packed result under the world's witness: every live sequence, dn, and the exact rest"""
    rat, kinds = aw.Ratios(), set()
    for b in w.seq:
        judge_seq(w, b, cut(w.wp, raw, b), rat, kinds)
    if raw.get("dn") is not None:
        gate_dn(w, raw["dn"], rat)
    exact_rest(w.wp, w, raw, rat)
    return rat, kinds


# ---------------------------------------------------------------- the item maps, in integers
def block_to_work(bid, nbh, nblk):
    """csrc/fasn_common.h block_to_work"""
    if nbh & 7 == 0:
        xcd, j = bid & 7, bid >> 3
        return (j // nblk) * 8 + xcd, j % nblk
    return bid // nblk, bid % nblk


def causal_head_group(nbh, rows, d):
    """csrc/fasn_common.h causal_head_group"""
    if nbh & 7:
        return 1
    hx, per_head, g = nbh >> 3, 4 * rows * d, 1
    while g < 4 and hx % (2 * g) == 0 and 2 * g * per_head <= (4 << 20):
        g *= 2
    return g


def block_to_work_grouped(bid, nbh, nblk, G):
    """csrc/fasn_common.h block_to_work_grouped"""
    if nbh & 7 == 0 and G > 1:
        xcd, j = bid & 7, bid >> 3
        per = G * nblk
        g, r = j // per, j % per
        return (g * G + r % G) * 8 + xcd, r // G
    return block_to_work(bid, nbh, nblk)


def item_model(wp, causal, hints=None):
    """The launches of csrc/fasn_attnvarlen.hip in integers. Per kernel ("fwd", "dq", "dkdv"): grid, nbh, nblk, G, aligned (the 8-aligned
    map) and items, the list of (sequence, head, block) the workgroups serve in launch order - the block already turned heaviest-first
    where the kernel does so (forward and dQ: causal; the dK/dV kernel walks its key blocks in order)."""
    p = wp.pack
    max_q, max_k = (p.max_q, p.max_k) if hints is None else hints
    nqblk, nkblk = -(-max_q // BLOCK), -(-max_k // BLOCK)
    kvg = wp.H // wp.Hkv
    out = {}
    nbh = p.B * wp.H
    items = []
    for bid in range(nqblk * nbh):
        bh, qi = block_to_work(bid, nbh, nqblk)
        items.append((bh // wp.H, bh % wp.H, nqblk - 1 - qi if causal else qi))
    out["fwd"] = dict(grid=nqblk * nbh, nbh=nbh, nblk=nqblk, G=1, aligned=nbh % 8 == 0, items=items)
    G = causal_head_group(nbh, p.Tk, D) if causal else 1
    items = []
    for bid in range(nqblk * nbh):
        bh, qi = block_to_work_grouped(bid, nbh, nqblk, G)
        items.append((bh // wp.H, bh % wp.H, nqblk - 1 - qi if causal else qi))
    out["dq"] = dict(grid=nqblk * nbh, nbh=nbh, nblk=nqblk, G=G, aligned=nbh % 8 == 0, items=items)
    nbk = p.B * wp.Hkv
    G = causal_head_group(nbk, p.Tq * kvg, D) if causal else 1
    items = []
    for bid in range(nkblk * (nbh // kvg)):
        bhk, kblk = block_to_work_grouped(bid, nbk, nkblk, G)
        items.append((bhk // wp.Hkv, bhk % wp.Hkv, kblk))
    out["dkdv"] = dict(grid=nkblk * nbk, nbh=nbk, nblk=nkblk, G=G, aligned=nbk % 8 == 0, items=items)
    return out


# ---------------------------------------------------------------- named plan cases (tests/golden/attn_varlen_witness_plans.txt)
VARIANTS = {
    "LONG8 self Hkv=4": lambda: long8(4), "LONG8 self Hkv=2": lambda: long8(2), "LONG8 self Hkv=1": lambda: long8(1),
    "LONG8 unequal Hkv=4": lambda: long8(4, True), "LONG8 unequal Hkv=2": lambda: long8(2, True), "LONG8 unequal Hkv=1": lambda: long8(1, True),
    "LONG4 H=8 Hkv=1": lambda: long4(8, 1), "LONG4 H=4 Hkv=4": lambda: long4(4, 4), "LONG4 H=3 Hkv=3": lambda: long4(3, 3),
    "MANY": lambda: many(),
}


def plans_file_text(pkg):
    """kernel names and grid sizes of every variant's forward and backward, through fasn_varlen_plan"""
    import ctypes
    lib = pkg._lib.load()
    buf = ctypes.create_string_buffer(1 << 14)
    out = []
    for name, make in VARIANTS.items():
        wp = make()
        p = wp.pack
        for causal in (False, True):
            for dtype, dn in ((torch.float16, "fp16"), (torch.bfloat16, "bf16")):
                a, vl = av.block(pkg, p.Tq, p.Tk, wp.H, wp.Hkv, D, dtype=dtype, causal=causal, n=0.0, num_seqs=p.B, max_q=p.max_q, max_k=p.max_k)
                for which, tag in ((0, "fwd"), (1, "bwd")):
                    rc = lib.fasn_varlen_plan(a, vl, which, buf, len(buf))
                    out.append(f"{name} {'causal' if causal else 'plain'} {dn} [{tag}] {'ok' if rc >= 0 else f'rc={rc}'}")
                    for line in buf.value.decode().splitlines():
                        kern, rest = line.rsplit(" grid=", 1)
                        out.append(f"    {kern} grid={rest.split()[0]}")
    return "\n".join(out) + "\n"
