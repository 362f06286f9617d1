"""What the tests of the decodes behind shared prefixes share (flash_attention_n_kvcache_shared_prefix / fasn_fwd_shared_prefix and
flash_attention_n_kvcache_prefix_groups / fasn_fwd_prefix_groups): the builder of the virtual cache behind G prefixes - `Groups`, and
`Shared`, its case of ONE prefix that every batch element is behind - its gather to dense per-sequence K / V, the runners of the parity
and the witness cases, the integer model of the schedule table and - for the suites without a GPU - the operands over fake pointers, the
named plan cases and the plan rules restated in Python. A plain module: no tests, importable without a GPU. It imports kv_support and
kv_witness and edits neither.

The virtual cache of batch element b with g = group[b] in [0, G) under P_g: key row j < P_g is row j % page of page
prefix_tables[g, j // page], key row j >= P_g is the row block_table[b] names; any other group value: the own rows alone. `Groups` builds
it from a dense picture kd / vd [B, Hkv, capacity, D]: the keys of prefix g are those of its FIRST member in batch order, which the dense
picture of every other member is overwritten with, so `kd` / `vd` of the object are what every batch element sees and the references
are computed on them.

What the memory contract lets hold anything does: the own slots of a member that lie wholly below P_g point at the poison page (NaN), its
own rows below P_g in the page that holds key P_g are NaN, the prefix pages' rows at or beyond P_g are NaN, a prefix table row's entries at
or beyond ceil(P_g / page) are the poison page, the WHOLE table row of a group without a member is the poison page, and - as in
kv_support._Paged - so is every row at or beyond len_b."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_args as ka        # noqa: E402
import kv_support as ks     # noqa: E402
import kv_witness as kw     # noqa: E402

NAN = float("nan")
GROUPS_MAX = 1024   # include/fasn.h: FASN_PREFIX_GROUPS_MAX


def effective(group, plens):
    """P_b of every batch element: the (already clamped) length of its group, 0 for a value outside [0, G)"""
    return [plens[g] if 0 <= g < len(plens) else 0 for g in group]


class Groups:
    """pool k / v, `table` [B, max_pages], `lens` [B], `prefix_tables` [G, prefix_pages], `plens` [G]
    and `group` [B] (device), and the dense virtual picture kd / vd. `plens`: the EFFECTIVE lengths (what the kernels clamp prefix_lens
    to); `group`: any integers, those outside [0, G) mean no prefix. `share`: the own tables name the prefix pages below P_b (page
    multiples) instead of the poison page - tables the base call can walk too."""

    def __init__(self, kd, vd, lens, group, plens, page, max_pages, seed, prefix_pages=None, alloc_all=False, share=False):
        B, Hkv, cap, D = kd.shape
        dev = kd.device
        G = len(plens)
        assert cap == page * max_pages and len(group) == B and len(lens) == B
        prefix_pages = prefix_pages or max_pages
        assert all(0 <= P <= min(prefix_pages * page, cap) for P in plens) and prefix_pages <= max_pages
        kd, vd = kd.clone(), vd.clone()
        first = [next((b for b in range(B) if group[b] == g), None) for g in range(G)]
        Pb = effective(group, plens)
        for b in range(B):
            if Pb[b]:
                f = first[group[b]]
                kd[b, :, :Pb[b]], vd[b, :, :Pb[b]] = kd[f, :, :Pb[b]], vd[f, :, :Pb[b]]
        # one pool: the B batch elements and, as elements B + g, the prefixes (their pages hold NaN at or beyond P_g, their table rows the
        # poison page beyond ceil(P_g / page); a group without a member owns no page at all)
        src = [f if f is not None else 0 for f in first]
        pc = ks._Paged(torch.cat([kd, kd[src]]), torch.cat([vd, vd[src]]), list(lens) + [P if f is not None else 0 for P, f in zip(plens, first)],
                       page, max_pages, seed, alloc_all=alloc_all)
        self.k, self.v, self.poison, self.page, self.max_pages = pc.k, pc.v, pc.poison, page, max_pages
        self.prefix_tables = pc.table[B:, :prefix_pages].clone().contiguous()
        for g in range(G):   # (under alloc_all a prefix owns what it needs: the rest is the poison page, as without alloc_all)
            self.prefix_tables[g, (-(-plens[g] // page) if first[g] is not None else 0):] = pc.poison
        self.table = pc.table[:B].clone()
        self.lens = pc.lens[:B].clone()
        self.lens_list, self.kd, self.vd = list(lens), kd, vd
        self.group_list, self.plens_list, self.Pb, self.G, self.first = list(group), list(plens), Pb, G, first
        for b in range(B):
            P = Pb[b]
            lo = (P // page) * page
            hi = min(P, cap if alloc_all else lens[b])
            for pos in range(lo, hi):   # own rows below P_b in the partially shared page
                pid = int(self.table[b, pos // page])
                self.k[pid, pos % page] = NAN
                self.v[pid, pos % page] = NAN
            if share and P:
                assert P % page == 0
                self.table[b, :P // page] = self.prefix_tables[group[b], :P // page]
            elif P:
                self.table[b, :P // page] = pc.poison
        self.plens = torch.tensor(plens, dtype=torch.int32, device=dev)
        self.group = torch.tensor([g if -2 ** 31 <= g < 2 ** 31 else -1 for g in group], dtype=torch.int32, device=dev)

    def gather(self, lens=None):
        """the virtual cache read through the tables as dense [B, Hkv, S, D] K and V; rows at or beyond len_b are zeros"""
        lens = self.lens_list if lens is None else lens
        dev = self.k.device
        need = max(1, max((ln + self.page - 1) // self.page for ln in lens))
        S = need * self.page
        j = torch.arange(S, device=dev).view(1, 1, S, 1)
        ln = torch.as_tensor(lens, device=dev).view(-1, 1, 1, 1)
        Pb = torch.as_tensor(self.Pb, device=dev).view(-1, 1, 1, 1)
        m = min(need, self.prefix_tables.shape[1])
        pt = torch.full((len(lens), need), self.poison, dtype=torch.long, device=dev)
        for b, g in enumerate(self.group_list):
            if self.Pb[b]:
                pt[b, :m] = self.prefix_tables[g, :m].long()
        res = []
        for pool in (self.k, self.v):
            own = pool[self.table[:, :need].long()].reshape(len(lens), S, pool.shape[2], pool.shape[3]).permute(0, 2, 1, 3)
            pre = pool[pt].reshape(len(lens), S, pool.shape[2], pool.shape[3]).permute(0, 2, 1, 3)
            d = torch.where(j < Pb, pre, own)
            res.append(torch.where(j < ln, d, torch.zeros_like(d)).contiguous())
        return res


class Shared(Groups):
    """Groups with G = 1 and every batch element in group 0: `prefix_table` [prefix_pages], `plen` [1] (device) and `P`, the effective
    prefix length, are the group fields of that one prefix - read-only views: a test that wants another table, length tensor or P
    writes into them in place (`sh.prefix_table[:] = ...`, `sh.plen.fill_(...)`) or builds another object; assigning to them raises."""

    def __init__(self, kd, vd, lens, P, page, max_pages, seed, prefix_pages=None, alloc_all=False, share=False):
        super().__init__(kd, vd, lens, [0] * kd.shape[0], [P], page, max_pages, seed, prefix_pages, alloc_all, share)

    prefix_table = property(lambda self: self.prefix_tables[0])
    plen = property(lambda self: self.plens)
    P = property(lambda self: self.plens_list[0])


def data(dev, B, H, Hkv, Sq, D, dtype, page, max_pages, seed):
    q = ks._rand((B, H, Sq, D), dtype, dev, seed)
    kd = ks._rand((B, Hkv, page * max_pages, D), dtype, dev, seed + 1)
    vd = ks._rand((B, Hkv, page * max_pages, D), dtype, dev, seed + 2, std=1.0)
    return q, kd, vd


def check(pkg, sh, out, lse, q, n, causal, dtype, what, lens=None, scale=None):
    """kv_support's gates on the gathered virtual cache, with flash_attention_n as second witness (ks._check_all)"""
    lens = sh.lens_list if lens is None else lens
    kg, vg = sh.gather(lens)
    return ks._check_all(pkg, out, lse, q, kg, vg, lens, [q.shape[2]] * q.shape[0], n, causal, dtype, what, True, scale)


def shared_call(pkg, sh, q, n, causal=True, prefix_len=None, **kw):
    return pkg.flash_attention_n_kvcache_shared_prefix(q, sh.k, sh.v, sh.lens, sh.table, sh.prefix_table, sh.plen if prefix_len is None else prefix_len,
                                                       softmax_n_param=n, is_causal=causal, return_lse=True, **kw)


def groups_call(pkg, gr, q, n, causal=True, prefix_lens=None, prefix_group=None, **kw):
    return pkg.flash_attention_n_kvcache_prefix_groups(q, gr.k, gr.v, gr.lens, gr.table, gr.prefix_tables,
                                                       gr.plens if prefix_lens is None else prefix_lens,
                                                       gr.group if prefix_group is None else prefix_group,
                                                       softmax_n_param=n, is_causal=causal, return_lse=True, **kw)


# ---------------------------------------------------------------- the witnesses of kv_witness behind shared prefixes
def witness_case(H, Hkv, D, Sq, lens, page=64, causal=True, max_pages=None):
    return kw.Case("decode", H, Hkv, D, Sq, lens, page=page, causal=causal, max_pages=max_pages)


def shared_witness_run(pkg, case, inp, P, seed=1):
    """kv_witness.run_decode behind a prefix of P keys: (the per-sequence rows, the inputs as every batch element sees them - the dense
    picture with the prefix of batch element 0 - for kv_witness.reference)"""
    sh = Shared(inp["kd"], inp["vd"], case.lens, P, case.page, case.max_pages, seed)
    out, lse = pkg.flash_attention_n_kvcache_shared_prefix(inp["q"], sh.k, sh.v, sh.lens, sh.table, sh.prefix_table, sh.plen,
                                                           softmax_n_param=inp["n"], scale=inp["scale"], is_causal=case.causal, return_lse=True)
    return kw._rows_of(case, out, lse, False), dict(inp, kd=sh.kd, vd=sh.vd)


def groups_witness_run(pkg, case, inp, group, plens, seed=1):
    """kv_witness.run_decode behind the prefixes `plens` with the batch elements assigned by `group`: (the per-sequence rows, the inputs as
    every batch element sees them, for kv_witness.reference)"""
    gr = Groups(inp["kd"], inp["vd"], case.lens, group, plens, case.page, case.max_pages, seed)
    out, lse = pkg.flash_attention_n_kvcache_prefix_groups(inp["q"], gr.k, gr.v, gr.lens, gr.table, gr.prefix_tables, gr.plens, gr.group,
                                                           softmax_n_param=inp["n"], scale=inp["scale"], is_causal=case.causal, return_lse=True)
    return kw._rows_of(case, out, lse, False), dict(inp, kd=gr.kd, vd=gr.vd)


# ---------------------------------------------------------------- the schedule table: its integer model and its place in the workspace
ROWS = 128   # rows of an item
HEAD = 4     # ints in front of the table's arrays


def items_max(B, R, G):
    return -(-B * R // ROWS) + min(G, B) - 1


def model(group, G, R, plens=None):
    """the table include/fasn.h documents, from the assignment alone: (order [B], slot [B], items [(group, first row, end row)], P_b [B],
    P_g of every item). Stable: by group, inside a group by batch index."""
    B = len(group)
    valid = [g if 0 <= g < G else -1 for g in group]
    order = [b for g in range(G) for b in range(B) if valid[b] == g]
    slot = [-1] * B
    for s, b in enumerate(order):
        slot[b] = s
    items, s0 = [], 0
    for g in range(G):
        c = sum(1 for v in valid if v == g)
        for i in range(-(-c * R // ROWS)):
            items.append((g, s0 * R + i * ROWS, (s0 + c) * R))
        s0 += c
    plens = plens if plens is not None else [0] * G
    return order + [-1] * (B - len(order)), slot, items, [plens[g] if g >= 0 else 0 for g in valid], [plens[it[0]] for it in items]


def table_ints(B, R, G):
    return HEAD + -(-3 * B // 4) * 4 + 4 * items_max(B, R, G)


def read_table(ws, partial_bytes, B, R, G):
    """the table of a workspace tensor (uint8) at its documented offset, as the tuple model() returns"""
    off = (partial_bytes + 15) // 16 * 16
    t = ws[off:off + 4 * table_ints(B, R, G)].view(torch.int32).cpu().tolist()
    n_items, n_grouped = t[0], t[1]
    assert t[2:4] == [0, 0] and 0 <= n_items <= items_max(B, R, G) and 0 <= n_grouped <= B
    at = HEAD + -(-3 * B // 4) * 4
    items = [tuple(t[at + 4 * i:at + 4 * i + 4]) for i in range(items_max(B, R, G))]
    assert all(it == (-1, 0, 0, 0) for it in items[n_items:]), "items beyond the count are not neutral"
    return (t[HEAD:HEAD + B], t[HEAD + B:HEAD + 2 * B], [it[:3] for it in items[:n_items]], t[HEAD + 2 * B:HEAD + 3 * B],
            [it[3] for it in items[:n_items]])


# ---------------------------------------------------------------- without a GPU: the operands over fake pointers, plan cases, the plan rules
def _prefix(pkg, pages=8, plen=ka.DUMMY + 256, table=ka.DUMMY + 512, reserved=0):
    return pkg._lib.SharedPrefix(prefix_len=plen, prefix_table=table, max_prefix_pages=pages, reserved=reserved)


def _groups(pkg, G=4, pages=8, lens=ka.DUMMY + 256, tables=ka.DUMMY + 512, group=ka.DUMMY + 1024, reserved=0):
    return pkg._lib.PrefixGroups(prefix_lens=lens, prefix_tables=tables, prefix_group=group, num_groups=G, max_prefix_pages=pages,
                                 reserved=reserved)


# name -> (the decode block's shape, max_prefix_pages)
SHARED_PLAN_CASES = {
    "gqa8_long_prefix": (dict(B=64, H=64, Hkv=8, Sq=1, page=256, max_pages=40), 32),
    "mha_long_prefix": (dict(B=64, H=16, Hkv=16, Sq=1, page=256, max_pages=40), 32),
    "gqa8_short_prefix": (dict(B=64, H=64, Hkv=8, Sq=1, page=256, max_pages=20), 4),
    "one_sequence": (dict(B=1, H=64, Hkv=8, Sq=1, page=256, max_pages=40), 32),
    "straddle": (dict(B=10, H=6, Hkv=2, Sq=5, page=64, max_pages=8), 3),
    "prefix_beyond_capacity": (dict(B=4, H=8, Hkv=2, Sq=4, page=64, max_pages=32), 48),
    "full_rows": (dict(B=3, H=64, Hkv=2, Sq=4, page=128, max_pages=64), 64),
}
# name -> (the decode block's shape, num_groups, max_prefix_pages)
GROUPS_PLAN_CASES = {
    "four_prompts_gqa8": (dict(B=64, H=64, Hkv=8, Sq=1, page=256, max_pages=40), 4, 32),
    "four_prompts_mha": (dict(B=64, H=16, Hkv=16, Sq=1, page=256, max_pages=40), 4, 32),
    "one_group": (dict(B=64, H=64, Hkv=8, Sq=1, page=256, max_pages=40), 1, 32),
    "nothing_shared": (dict(B=64, H=64, Hkv=8, Sq=1, page=256, max_pages=40), 64, 32),
    "more_groups_than_sequences": (dict(B=3, H=8, Hkv=2, Sq=4, page=64, max_pages=8), 16, 3),
    "straddle": (dict(B=13, H=6, Hkv=2, Sq=5, page=64, max_pages=8), 2, 4),
    "groups_at_the_limit": (dict(B=2048, H=8, Hkv=8, Sq=1, page=64, max_pages=16), GROUPS_MAX, 8),
    "prefix_beyond_capacity": (dict(B=4, H=8, Hkv=2, Sq=4, page=64, max_pages=32), 2, 48),
}


def _plan(B, H, Hkv, Sq, D, page, max_pages, prefix_pages, units):
    """what the two rules share, `units` being the 128-row units the prefix pass has workgroups for: (grid of the prefix pass, of the
    suffix pass, of the combine, bytes of the partials) as include/fasn.h states them"""
    R = (H // Hkv) * Sq
    cap = page * max_pages
    target = 1024
    nsplit = max(1, min(-(-target // (B * Hkv)), -(-cap // 64) // max(4, R // 8)))
    pcap = min(prefix_pages * page, cap)
    nsplit_p = max(1, min(-(-target // (Hkv * units)), -(-pcap // 64) // 16))
    partials = (B * Hkv * nsplit * R + Hkv * nsplit_p * B * R) * (D + 2) * 4
    return Hkv * units * nsplit_p, B * Hkv * nsplit, -(-B * Hkv * R * (D // 4) // 256), partials


def shared_plan_rule(B, H, Hkv, Sq, D, page, max_pages, prefix_pages):
    """(grid of the prefix pass, of the suffix pass, of the combine, workspace bytes): the units are the blocks of the row space"""
    return _plan(B, H, Hkv, Sq, D, page, max_pages, prefix_pages, -(-B * (H // Hkv) * Sq // ROWS))


def groups_plan_rule(B, H, Hkv, Sq, D, page, max_pages, G, prefix_pages):
    """(grid of the prefix pass, of the suffix pass, of the combine, bytes of the partials, workspace bytes): the units are the most items
    a table can hold, the table lies behind the partials; the schedule kernel is one workgroup"""
    R = (H // Hkv) * Sq
    plan = _plan(B, H, Hkv, Sq, D, page, max_pages, prefix_pages, items_max(B, R, G))
    return (*plan, (plan[3] + 15) // 16 * 16 + 4 * table_ints(B, R, G))


def lds_bytes(D):
    return 2 * (3 if D <= 64 else 2) * 64 * D * 2
