"""What the shared-prefix decode tests share (flash_attention_n_kvcache_shared_prefix / fasn_fwd_shared_prefix): the builder of the virtual
cache, its gather to dense per-sequence K / V, the runners of the parity and the witness cases, and - for the suite without a GPU - the
prefix operand over fake pointers, the named plan cases and the plan rule restated in Python. A plain module: no tests, importable
without a GPU. It imports kv_support and kv_witness and edits neither.

The virtual cache of batch element b under a prefix of P keys: key row j < P is row j % page of page prefix_table[j // page], key row
j >= P is the row block_table[b] names. `Shared` builds it from a dense picture kd / vd [B, Hkv, capacity, D]: the prefix's keys are those
of batch element 0 (kd[0, :, :P]), which the dense picture of every other batch element is overwritten with, so `kd` / `vd` of the object
are what every batch element sees and the references are computed on them.

What the memory contract lets hold anything does: the own slots of a batch element that lie wholly below P point at the poison page
(NaN), its own rows below P in the page that holds key P are NaN, the prefix pages' rows at or beyond P are NaN, the prefix table's
entries at or beyond ceil(P / page) are the poison page, and - as in kv_support._Paged - so is every row at or beyond len_b."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_args as ka        # noqa: E402
import kv_support as ks     # noqa: E402
import kv_witness as kw     # noqa: E402

NAN = float("nan")


class Shared:
    """pool k / v, `table` [B, max_pages], `lens` [B] (device), `prefix_table` [prefix_pages], and the dense virtual picture kd / vd.
    `P`: the effective prefix length (what the kernels clamp prefix_len to). `share`: the own tables name the prefix pages below P (P a
    page multiple) instead of the poison page - the tables a server has today, which the base call can walk too."""

    def __init__(self, kd, vd, lens, P, page, max_pages, seed, prefix_pages=None, alloc_all=False, share=False):
        B, Hkv, cap, D = kd.shape
        dev = kd.device
        assert cap == page * max_pages and 0 <= P <= cap
        prefix_pages = prefix_pages or max_pages
        assert P <= prefix_pages * page and prefix_pages <= max_pages
        kd, vd = kd.clone(), vd.clone()
        kd[:, :, :P], vd[:, :, :P] = kd[0:1, :, :P], vd[0:1, :, :P]
        # one pool: the B batch elements and, as element B, the prefix (its pages hold NaN at or beyond P, its table the poison page
        # beyond ceil(P / page))
        pc = ks._Paged(torch.cat([kd, kd[0:1]]), torch.cat([vd, vd[0:1]]), list(lens) + [P], page, max_pages, seed, alloc_all=alloc_all)
        self.k, self.v, self.poison, self.page, self.max_pages = pc.k, pc.v, pc.poison, page, max_pages
        self.prefix_table = pc.table[B, :prefix_pages].clone()
        if alloc_all:   # (the prefix owns what it needs: the rest is the poison page, as without alloc_all)
            self.prefix_table[-(-P // page):] = pc.poison
        self.table = pc.table[:B].clone()
        self.lens = pc.lens[:B].clone()
        self.lens_list, self.P, self.kd, self.vd = list(lens), P, kd, vd
        for b in range(B):
            lo = (P // page) * page
            hi = min(P, cap if alloc_all else lens[b])
            for pos in range(lo, hi):   # own rows below P in the partially shared page
                pid = int(self.table[b, pos // page])
                self.k[pid, pos % page] = NAN
                self.v[pid, pos % page] = NAN
            if share:
                assert P % page == 0
                self.table[b, :P // page] = self.prefix_table[:P // page]
            else:
                self.table[b, :P // page] = pc.poison
        self.plen = torch.tensor([P], dtype=torch.int32, device=dev)

    def gather(self, lens=None):
        """the virtual cache read through the two tables as dense [B, Hkv, S, D] K and V; rows at or beyond len_b are zeros"""
        lens = self.lens_list if lens is None else lens
        need = max(1, max((ln + self.page - 1) // self.page for ln in lens))
        S = need * self.page
        j = torch.arange(S, device=self.k.device).view(1, 1, S, 1)
        ln = torch.as_tensor(lens, device=self.k.device).view(-1, 1, 1, 1)
        pt = torch.full((need,), self.poison, dtype=torch.long, device=self.k.device)
        m = min(need, self.prefix_table.shape[0])
        pt[:m] = self.prefix_table[:m].long()
        res = []
        for pool in (self.k, self.v):
            own = pool[self.table[:, :need].long()].reshape(len(lens), S, pool.shape[2], pool.shape[3]).permute(0, 2, 1, 3)
            pre = pool[pt].reshape(1, S, pool.shape[2], pool.shape[3]).permute(0, 2, 1, 3).expand_as(own)
            d = torch.where(j < self.P, pre, own)
            res.append(torch.where(j < ln, d, torch.zeros_like(d)).contiguous())
        return res


def data(dev, B, H, Hkv, Sq, D, dtype, page, max_pages, seed):
    q = ks._rand((B, H, Sq, D), dtype, dev, seed)
    kd = ks._rand((B, Hkv, page * max_pages, D), dtype, dev, seed + 1)
    vd = ks._rand((B, Hkv, page * max_pages, D), dtype, dev, seed + 2, std=1.0)
    return q, kd, vd


def call(pkg, sh, q, n, causal=True, prefix_len=None, **kw):
    return pkg.flash_attention_n_kvcache_shared_prefix(q, sh.k, sh.v, sh.lens, sh.table, sh.prefix_table, sh.plen if prefix_len is None else prefix_len,
                                                       softmax_n_param=n, is_causal=causal, return_lse=True, **kw)


def check(pkg, sh, out, lse, q, n, causal, dtype, what, lens=None, scale=None):
    """kv_support's gates on the gathered virtual cache, with flash_attention_n as second witness (ks._check_all)"""
    lens = sh.lens_list if lens is None else lens
    kg, vg = sh.gather(lens)
    return ks._check_all(pkg, out, lse, q, kg, vg, lens, [q.shape[2]] * q.shape[0], n, causal, dtype, what, True, scale)


# ---------------------------------------------------------------- the witnesses of kv_witness behind a shared prefix
def witness_case(H, Hkv, D, Sq, lens, page=64, causal=True, max_pages=None):
    return kw.Case("decode", H, Hkv, D, Sq, lens, page=page, causal=causal, max_pages=max_pages)


def witness_run(pkg, case, inp, P, seed=1):
    """kv_witness.run_decode behind a prefix of P keys: (the per-sequence rows, the inputs as every batch element sees them - the dense
    picture with the prefix of batch element 0 - for kv_witness.reference)"""
    sh = Shared(inp["kd"], inp["vd"], case.lens, P, case.page, case.max_pages, seed)
    out, lse = pkg.flash_attention_n_kvcache_shared_prefix(inp["q"], sh.k, sh.v, sh.lens, sh.table, sh.prefix_table, sh.plen,
                                                           softmax_n_param=inp["n"], scale=inp["scale"], is_causal=case.causal, return_lse=True)
    return kw._rows_of(case, out, lse, False), dict(inp, kd=sh.kd, vd=sh.vd)


# ---------------------------------------------------------------- without a GPU: the operand over fake pointers, plan cases, the plan rule
def _prefix(pkg, pages=8, plen=ka.DUMMY + 256, table=ka.DUMMY + 512, reserved=0):
    return pkg._lib.SharedPrefix(prefix_len=plen, prefix_table=table, max_prefix_pages=pages, reserved=reserved)


# name -> (the decode block's shape, max_prefix_pages)
PLAN_CASES = {
    "gqa8_long_prefix": (dict(B=64, H=64, Hkv=8, Sq=1, page=256, max_pages=40), 32),
    "mha_long_prefix": (dict(B=64, H=16, Hkv=16, Sq=1, page=256, max_pages=40), 32),
    "gqa8_short_prefix": (dict(B=64, H=64, Hkv=8, Sq=1, page=256, max_pages=20), 4),
    "one_sequence": (dict(B=1, H=64, Hkv=8, Sq=1, page=256, max_pages=40), 32),
    "straddle": (dict(B=10, H=6, Hkv=2, Sq=5, page=64, max_pages=8), 3),
    "prefix_beyond_capacity": (dict(B=4, H=8, Hkv=2, Sq=4, page=64, max_pages=32), 48),
    "full_rows": (dict(B=3, H=64, Hkv=2, Sq=4, page=128, max_pages=64), 64),
}


def plan_rule(B, H, Hkv, Sq, D, page, max_pages, prefix_pages):
    """(grid of the prefix pass, of the suffix pass, of the combine, workspace bytes) as include/fasn.h states them"""
    R = (H // Hkv) * Sq
    cap = page * max_pages
    target = 1024
    nsplit = max(1, min(-(-target // (B * Hkv)), -(-cap // 64) // max(4, R // 8)))
    nrb = -(-B * R // 128)
    pcap = min(prefix_pages * page, cap)
    nsplit_p = max(1, min(-(-target // (Hkv * nrb)), -(-pcap // 64) // 16))
    ws = (B * Hkv * nsplit * R + Hkv * nsplit_p * B * R) * (D + 2) * 4
    return Hkv * nrb * nsplit_p, B * Hkv * nsplit, -(-B * Hkv * R * (D // 4) // 256), ws


def lds_bytes(D):
    return 2 * (3 if D <= 64 else 2) * 64 * D * 2
