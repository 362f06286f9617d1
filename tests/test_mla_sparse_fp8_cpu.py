"""Sparse MLA decode over 656-byte FP8 rows without a GPU: pack / unpack and the scale rule in plain torch; what the entry points and the
Python calls refuse on a block read in bytes (fasn_fwd_mla_sparse's own refusals are test_mla_sparse_cpu's); plan and workspace."""
import ctypes

import pytest
import torch

from mla_support import BASE, EALIGN, EINVAL, EUNSUPPORTED, _args, _block, _sparse


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_pack_unpack_and_the_scale_rule(pkg, dtype):
    pack, unpack = pkg.mla_fp8_rows_pack, pkg.mla_fp8_rows_unpack
    # every finite e4m3 code times a power of two per group, the code 448 in each group: unpack(pack(x)) is x, the scale is that power
    codes = torch.tensor([c for c in range(256) if c & 0x7F != 0x7F], dtype=torch.uint8).view(torch.float8_e4m3fn).float()
    lat = codes[torch.randint(0, 254, (7, 512), generator=torch.Generator().manual_seed(1))]
    lat[:, ::128] = 448.0
    pw = torch.tensor([2.0 ** -6, 1.0, 2.0 ** 3, 2.0 ** -1]).repeat_interleave(128)
    x = torch.cat([lat * pw, torch.randn(7, 64)], -1).to(dtype)
    rows = pack(x)
    assert rows.dtype == torch.uint8 and rows.shape == (7, 656) and torch.equal(unpack(rows.view(torch.float8_e4m3fn), dtype).view(torch.int16), x.view(torch.int16))
    assert torch.equal(rows[:, 512:528].contiguous().view(torch.float32), pw[::128].expand(7, 4))
    # the scale at a = 0, a = 448 * 2^k and the next 16-bit number above it; NaN and Inf stay out of the amax, clamp or give the NaN code
    top, y = torch.tensor([448.0 * 2.0 ** -5], dtype=dtype), torch.zeros(3, 576, dtype=dtype)
    y[1, 5], y[1, 128 + 9], y[1, 256] = top[0], (top.view(torch.int16) + 1).view(dtype)[0], 3.0
    y[2, :4] = torch.tensor([float("nan"), float("inf"), float("-inf"), 1.0], dtype=dtype)
    r = pack(y)
    s = r[:, 512:528].contiguous().view(torch.float32)
    assert torch.equal(s[0], torch.full((4,), 2.0 ** -30)) and not r[0, :512].any()
    assert s[1].tolist() == [2.0 ** -5, 2.0 ** -4, 2.0 ** -7, 2.0 ** -30] and r[1, 5] == 0x7E and r[1, 128 + 9] == 0x76   # 448; 224 under twice the scale
    assert s[2, 0] == 2.0 ** -8 and r[2, :4].tolist() == [0x7F, 0x7E, 0xFE, 0x78]


REFUSALS = [   # (what, block, list, code)
    ("a 16-bit cache's row stride (576 < 656)", dict(stride=(64 * 576, 576)), dict(), EINVAL),
    ("row stride off 16 bytes", dict(stride=(64 * 664, 664)), dict(), EALIGN),
    ("fp16 scale 6", dict(dtype=0, scale=6.0), dict(), EUNSUPPORTED),
    ("topk 96", dict(), dict(topk=96), EUNSUPPORTED),
    ("the block before the list: row stride off 16 bytes, topk 96", dict(stride=(64 * 664, 664)), dict(topk=96), EALIGN),
]


@pytest.mark.parametrize("what,over,sover,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_entry_points_refuse_with_the_headers_codes(pkg, what, over, sover, code):
    lib, buf, a, s = pkg._lib.load(), ctypes.create_string_buffer(4096), _block(pkg, **over), ctypes.byref(_sparse(pkg, **sover))
    assert (lib.fasn_fwd_mla_sparse_fp8(a, s, BASE, 0, None), lib.fasn_mla_sparse_fp8_plan(a, s, buf, len(buf)), lib.fasn_mla_sparse_fp8_workspace_bytes(a, s)) == (code, code, 0), what
    if not sover:   # the block itself is refused: so is its append, which has no list and looks at the block first (a served one would launch)
        assert lib.fasn_mla_sparse_fp8_append(a, None, None) == code, what


@pytest.mark.parametrize("B,H,Sq,topk", [(2, 16, 2, 2048), (3, 65, 1, 64)])
def test_plan_and_workspace_are_the_16_bit_sparse_calls(pkg, B, H, Sq, topk):
    s, a8, a16 = _sparse(pkg, topk=topk, stride_b=Sq * topk, stride_q=topk), _block(pkg, B=B, H=H, Sq=Sq), _args(pkg, B=B, H=H, Sq=Sq)
    plan, plan16, lib = pkg._lib.mla_sparse_fp8_plan(a8, s), pkg._lib.mla_sparse_plan(a16, s), pkg._lib.load()
    assert [k[0].split("<")[0] for k in plan] == ["fasn_mla_sparse_fp8_fwd_kernel", "fasn_mla_combine_kernel"]
    assert plan[0][1:3] == plan16[0][1:3] and plan[0][3] == 2 * 64 * 656 + 64 * 1152 and plan[1] == plan16[1] and lib.fasn_mla_sparse_fp8_workspace_bytes(a8, s) == lib.fasn_mla_sparse_workspace_bytes(a16, s) > 0
    assert lib.fasn_fwd_mla_sparse_fp8(a8, s, BASE, 0, None) == -8   # the workspace comes behind every check


def test_python_calls_name_what_is_served(pkg):
    new, old, u8, f8 = pkg.flash_attention_n_mla_sparse_fp8, pkg.flash_attention_n_mla_sparse, torch.uint8, torch.float8_e4m3fn
    assert {"flash_attention_n_mla_sparse_fp8", "mla_fp8_rows_pack", "mla_fp8_rows_unpack"} <= set(pkg.__all__)
    q, rows = torch.zeros(1, 4, 2, 576, dtype=torch.float16), torch.zeros(2, 64, 1, 656, dtype=u8)
    lens, table, idx = torch.zeros(1, dtype=torch.int32), torch.zeros(1, 1, dtype=torch.int32), torch.zeros(1, 2, 64, dtype=torch.int32)
    for fn, cache, ind, scale, err, pattern in (
            (new, torch.zeros(2, 64, 1, 576, dtype=u8), idx, 0.1, ValueError, "not a latent cache.*served: .*656-byte"),
            (new, torch.zeros(2, 64, 1, 664, dtype=u8)[..., :656], idx, 0.1, ValueError, "16-byte aligned"),
            (new, torch.zeros(2, 64, 1, 576, dtype=torch.float16), idx, 0.1, TypeError, "656-byte rows as torch.uint8.*is flash_attention_n_mla_sparse's"),
            (new, rows, idx[..., :32].repeat(1, 1, 3), 0.1, ValueError, "topk = 96.*served: "),
            (new, rows, idx, 6.0, ValueError, "log2\\(e\\) <= 8"),
            (new, rows.view(f8), idx, 0.1, RuntimeError, "no CPU fallback"),
            (old, rows, idx, 0.1, TypeError, "behind indices is flash_attention_n_mla_sparse_fp8's.*served: .*top-k list")):
        with pytest.raises(err, match=pattern):
            fn(q, cache, ind, lens, scale, block_table=table)
