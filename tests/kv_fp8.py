"""What the FP8 K/V-cache tests share: the FP8 operand over fake pointers (plans and refusals), the quantisation reference of the append
and the brute-force nearest-code search it is checked against, the witnesses of the append, code tensors and a paged cache of codes with
NaN codes (0x7f) in every stale row and page, and the 16-bit call the FP8 call must equal bit for bit under power-of-two scales.
A plain module: no tests, importable without a GPU."""
import torch

import kv_args

DUMMY = kv_args.DUMMY
F8 = torch.float8_e4m3fn
E4M3_MAX = 448.0
NAN_CODE = 0x7F
POW2_SCALES = (1.0, 2.0 ** -3, 2.0 ** 4)   # the scales of the exactness witnesses


# ---------------------------------------------------------------- operand and argument blocks (fake pointers)
def _fp8(pkg, k_scale=DUMMY + 1024, v_scale=DUMMY + 2048, sb=0, sh=1, reserved=0):
    o = pkg._lib.KvFp8()
    o.k_scale, o.v_scale = k_scale, v_scale
    o.k_sb, o.k_sh, o.v_sb, o.v_sh = sb, sh, sb, sh
    o.reserved = reserved
    return o


def fp8_plan(pkg, args, op=None):
    return pkg._lib.kvfp8_plan(args, _fp8(pkg) if op is None else op)


# ---------------------------------------------------------------- codes
def all_codes():
    """the 256 codes as uint8, and their values in fp64 (NaN for 0x7f / 0xff)"""
    c = torch.arange(256, dtype=torch.uint8)
    return c, c.view(F8).double()


def finite_codes():
    c, v = all_codes()
    keep = ~torch.isnan(v)
    assert int(keep.sum()) == 254
    return c[keep], v[keep]


def is_nan_code(b):
    return (b & 0x7F) == NAN_CODE


def up(codes_u8, dtype=torch.float32):
    """the exact upcast of uint8 codes"""
    return codes_u8.view(F8).to(dtype)


# ---------------------------------------------------------------- the append's reference
def quantise(x, s):
    """code = rne_e4m3(clamp(float(x) / s, -448, 448)) as uint8, on the CPU: the fp32 division is IEEE there, the clamp comes BEFORE the
    cast (torch's cast does not saturate: 500 -> NaN) and lets a NaN through. `s` broadcasts against x."""
    y = x.detach().cpu().float() / torch.as_tensor(s, dtype=torch.float32).cpu()
    y = torch.where(y > E4M3_MAX, torch.full_like(y, E4M3_MAX), torch.where(y < -E4M3_MAX, torch.full_like(y, -E4M3_MAX), y))
    return y.to(F8).view(torch.uint8)


def nearest_code(y):
    """Brute force, independent of torch's cast: for each fp32 y (already divided) the finite code nearest to clamp(y, -448, 448) in exact
    fp64 arithmetic, a tie going to the code with an even mantissa, a zero result keeping the sign of y; NaN -> 0x7f."""
    codes, vals = finite_codes()
    out = torch.empty(y.numel(), dtype=torch.uint8)
    flat = y.detach().cpu().double().reshape(-1)
    for i, t in enumerate(flat.tolist()):
        if t != t:
            out[i] = NAN_CODE
            continue
        neg = torch.tensor(t).signbit().item()
        t = min(max(t, -E4M3_MAX), E4M3_MAX)
        d = (vals - t).abs()
        best = d.min()
        cand = codes[d == best]
        cand = cand[((cand & 0x80) != 0) == neg]   # +0 and -0 are one value: the sign of y decides (no other code of the wrong sign is nearest)
        if cand.numel() > 1:   # a tie between two neighbours: the even mantissa
            cand = cand[(cand & 1) == 0]
        assert cand.numel() == 1, (t, cand)
        out[i] = cand[0]
    return out.view(y.shape)


def append_witnesses(dtype):
    """values (at scale 1) the append must get right, as a 1-D tensor in `dtype`: ties between neighbouring codes (normal and subnormal),
    every subnormal, both zeros, values at and beyond +-448 (saturation: 0x7e / 0xfe), infinities, NaN. All are fp16 and bf16 numbers
    except where the cast to `dtype` rounds them, which is part of the input then."""
    v = [0.0, -0.0, 1.0, 1.0625, 1.125, 1.1875, 1.25, -1.0625, -1.1875, 0.9375 + 2.0 ** -5, 3.25, 3.75, 416.0, 432.0, 448.0, 449.0, 464.0, 480.0,
         500.0, 1e4, 65504.0, -448.0, -464.0, -500.0, -1e4, float("inf"), float("-inf"), float("nan")]
    v += [k * 2.0 ** -9 for k in range(1, 9)] + [-(k * 2.0 ** -9) for k in range(1, 9)]                 # the subnormals and the first normal
    v += [(2 * k + 1) * 2.0 ** -10 for k in range(0, 8)] + [-((2 * k + 1) * 2.0 ** -10) for k in range(0, 8)]   # ties between them
    v += [2.0 ** -11, -(2.0 ** -11), 2.0 ** -10 + 2.0 ** -13, 2.0 ** -12, 1e-7, -1e-7]                   # below the first tie, just above it
    return torch.tensor(v, dtype=torch.float32).to(dtype)


# ---------------------------------------------------------------- data on the device
def rand_codes(shape, seed, dev, top=0x48):
    """random finite codes, |value| <= up(top) (0x48: 3.0), either sign"""
    gen = torch.Generator().manual_seed(seed)
    mag = torch.randint(0, top + 1, shape, generator=gen, dtype=torch.int32)
    sign = torch.randint(0, 2, shape, generator=gen, dtype=torch.int32) << 7
    return (mag | sign).to(torch.uint8).to(dev)


class PagedCodes:
    """A paged cache of codes built from dense [B, Hkv, Smax, D] uint8 codes: shuffled page ids; every row at or beyond len_b inside a
    needed page is the NaN code, every table entry beyond the needed pages names a poison page of NaN codes, and spare pages no table
    names are NaN codes too. `k` / `v` are the float8 views the call takes, `ku` / `vu` the same memory as uint8."""

    def __init__(self, kd, vd, lens, page, max_pages, seed, spare=2):
        B, Hkv, Smax, D = kd.shape
        dev = kd.device
        assert Smax == page * max_pages
        need = [(ln + page - 1) // page for ln in lens]
        n_ids = sum(need) + spare + 1
        ids = torch.randperm(n_ids, generator=torch.Generator().manual_seed(seed)).tolist()
        self.poison = ids.pop()
        self.ku = torch.full((n_ids, page, Hkv, D), NAN_CODE, dtype=torch.uint8, device=dev)
        self.vu = torch.full((n_ids, page, Hkv, D), NAN_CODE, dtype=torch.uint8, device=dev)
        table = torch.full((B, max_pages), self.poison, dtype=torch.int32)
        for b in range(B):
            for s in range(need[b]):
                pid = ids.pop()
                table[b, s] = pid
                rows = max(0, min(page, lens[b] - s * page))
                if rows:
                    self.ku[pid, :rows] = kd[b, :, s * page:s * page + rows].transpose(0, 1)
                    self.vu[pid, :rows] = vd[b, :, s * page:s * page + rows].transpose(0, 1)
        self.k, self.v = self.ku.view(F8), self.vu.view(F8)
        self.table = table.to(dev)
        self.lens = torch.tensor(lens, dtype=torch.int32, device=dev)
        self.page, self.max_pages = page, max_pages


def visible(codes_dense, lens):
    """dense [B, Hkv, S, D] uint8 codes with the rows at or beyond len_b set to code 0 (+0)"""
    keep = torch.arange(codes_dense.shape[2], device=codes_dense.device).view(1, 1, -1, 1) < torch.as_tensor(lens, device=codes_dense.device).view(-1, 1, 1, 1)
    return torch.where(keep, codes_dense, torch.zeros_like(codes_dense))


def scales_bh(values, B, Hkv, dev, seed):
    """a [B, Hkv] fp32 tensor drawn from `values`, every value present when B * Hkv allows"""
    gen = torch.Generator().manual_seed(seed)
    idx = torch.cat([torch.arange(len(values)), torch.randint(0, len(values), (max(0, B * Hkv - len(values)),), generator=gen)])[:B * Hkv]
    idx = idx[torch.randperm(B * Hkv, generator=gen)]
    return torch.tensor(values, dtype=torch.float32)[idx].view(B, Hkv).to(dev)


def sixteen_bit_twin(call16, q, k16, v16, k_scale, v_scale, scale, **kw):
    """What the FP8 call must equal bit for bit when every scale is a power of two: `call16` (the 16-bit cache call of the same route) on
    the exactly upcast cache with scale * k_scale, its out times v_scale. The 16-bit call takes one scale per call, so it runs once per
    distinct k_scale and each (b, hkv) takes its rows from the run of its own scale. Returns (the 16-bit out as fp32, v_scale per query
    head [B, H], lse): the product is left to assert_bitwise, which knows where it is exact."""
    B, H, Sq, D = q.shape
    Hkv = k16.shape[2]
    G = H // Hkv
    scale = D ** -0.5 if scale is None else scale
    ks_h = k_scale.repeat_interleave(G, dim=1)    # [B, H]
    out = torch.zeros(B, H, Sq, D, dtype=torch.float32, device=q.device)
    lse = torch.zeros(B, H, Sq, dtype=torch.float32, device=q.device)
    for u in sorted(set(k_scale.flatten().tolist())):
        o_u, l_u = call16(q, k16, v16, scale=scale * u, return_lse=True, **kw)
        pick = (ks_h == u)
        out = torch.where(pick[:, :, None, None], o_u.float(), out)
        lse = torch.where(pick[:, :, None], l_u, lse)
    return out, v_scale.repeat_interleave(G, dim=1), lse


def assert_bitwise(got, out16, vs_h, got_lse, want_lse, dtype, what):
    """`got` (16-bit) against the twin: the 16-bit call's out (as fp32) times the power of two v_scale. A 16-bit number times a power of two
    is exact, and so is the twin, wherever both the 16-bit call's own result and the product are normal numbers of `dtype` (or zero): there
    the bits must agree. fp16 only: below 2^-14 a number is subnormal and was rounded on the grid of 2^-24, not to 11 bits - the twin has
    then rounded once more than the FP8 call, or on a coarser grid than the product's (v_scale > 1). There the twin's own error, one
    subnormal ulp on either side of the scaling, is the bound, and such elements must be rare."""
    tiny = 2.0 ** -14 if dtype == torch.float16 else 2.0 ** -126
    vs = vs_h[:, :, None, None]
    want32 = out16 * vs
    want = want32.to(dtype)
    exact = ((out16.abs() >= tiny) & (want32.abs() >= tiny)) | ((out16 == 0) & (got == 0))   # (a row that sees nothing is 0 on both sides)
    same = got.view(torch.int16) == want.view(torch.int16)
    both_nan = torch.isnan(got) & torch.isnan(want)
    bad = exact & ~(same | both_nan)
    print(f"{what}: {int((~exact).sum())} of {exact.numel()} elements in the subnormal range of {dtype}, {int(bad.sum())} mismatches elsewhere")
    where = [(idx, float(got[tuple(idx)]), float(want[tuple(idx)])) for idx in bad.nonzero()[:8].tolist()]
    assert not bad.any(), f"{what}: out differs from the 16-bit call at {int(bad.sum())} elements; (index, got, want): {where}"
    assert (~exact).float().mean().item() <= 0.05, f"{what}: too many subnormal results for an exact comparison"
    if (~exact).any():
        over = ((got.float() - want32).abs() - 2.0 ** -24 * vs.clamp_min(1.0).expand_as(want32))[~exact].max().item()
        assert over <= 0, f"{what}: a result in the subnormal range is off by more than the twin's own rounding"
    eq = (got_lse == want_lse) | (torch.isnan(got_lse) & torch.isnan(want_lse))
    assert eq.all(), f"{what}: lse differs from the 16-bit call at {int((~eq).sum())} rows, max {(got_lse - want_lse)[~eq].abs().max().item():.3e}"
