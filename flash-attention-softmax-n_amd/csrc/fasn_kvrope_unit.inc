// fasn_kvrope_unit.inc - the rotation of ONE UNIT of a row, the text fasn_kvrope_kernel and fasn_kvvarlen_rope_kernel share (included by
// fasn_kvrope.h inside both kernels, no include guard; the family's way - fasn_kvprefill_fwd.inc - rather than a function: an inlined
// function gives the padded kernel other device code than it had, this text gives it the same). In scope at the point of inclusion:
//   Tag, rp (KvRopeParams), u (the lane's unit), src / dst (the row's first byte in the source and the destination), pos (its position).
// Chunks c1 / c2 of src go to dst: rotated at table row clamp(pos, 0, rows - 1) when u is a rotated unit, copied otherwise. The kernel
// ends here.
// FASN_KVROPE_FP8 = 1 (fasn_kvfp8.h: fasn_kvrope_fp8_kernel; undefined counts as 0): a K/V unit (!isq) stores chunk c - the 16-bit values
// every other kernel stores - as their 8 e4m3fn codes under the scale `ksc` at byte 8 c of the code row `dst8`; E = ET<Tag> is in scope
// too. The store has one name for that; with FASN_KVROPE_FP8 == 0 it is the 16-byte store it was, token for token.
// FASN_KVROPE_INVERSE = 1 (fasn_varlen_rope.hip: the packed training call, whose backward rotates gradients; undefined counts as 0):
// `rp.inverse` != 0 negates the sines behind the table read. With FASN_KVROPE_INVERSE == 0 no token is added.
#if FASN_KVROPE_FP8
#define FASN_KVROPE_STORE(c, x)                                        \
    do {                                                               \
        if (isq) gstore16(dst + c * 16, x);                            \
        else gstore8(dst8 + c * 8, kv_fp8_quant8<E>(x, ksc));          \
    } while (0)
#else
#define FASN_KVROPE_STORE(c, x) gstore16(dst + c * 16, x)
#endif
    const int ru = rp.rd / 16;   // rotated units
    const bool rot = u < ru;
    const int c1 = rot && !rp.interleaved ? u : 2 * u, c2 = rot && !rp.interleaved ? u + ru : 2 * u + 1;
    const u32x4 a = gload16(src + c1 * 16), bq = gload16(src + c2 * 16);
    if (!rot) {
        FASN_KVROPE_STORE(c1, a);
        FASN_KVROPE_STORE(c2, bq);
        return;
    }
    const int64_t trow = min(max(pos, (int64_t)0), (int64_t)rp.rows - 1);
    float c[8], s[8], e0[8], e1[8], x1[8], x2[8], y1[8], y2[8];
    kvrope_table<Tag>(rp.cos, trow * rp.trs + 8 * u, rp.tf32, c);
    kvrope_table<Tag>(rp.sin, trow * rp.trs + 8 * u, rp.tf32, s);
#if FASN_KVROPE_INVERSE
    if (rp.inverse) {   // the transpose rotation: sin negated, which is exact - y1 = x1 c + x2 s, y2 = x2 c - x1 s with the same roundings
#pragma unroll
        for (int j = 0; j < 8; ++j) s[j] = -s[j];
    }
#endif
    kvrope_widen<Tag>(a, e0);
    kvrope_widen<Tag>(bq, e1);
    if (rp.interleaved) {   // the 16 elements are the pairs (2 j, 2 j + 1)
#pragma unroll
        for (int j = 0; j < 4; ++j) x1[j] = e0[2 * j], x2[j] = e0[2 * j + 1], x1[4 + j] = e1[2 * j], x2[4 + j] = e1[2 * j + 1];
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) x1[j] = e0[j], x2[j] = e1[j];
    }
    {
#pragma clang fp contract(off)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float ac = x1[j] * c[j], bs = x2[j] * s[j], bc = x2[j] * c[j], as = x1[j] * s[j];
            y1[j] = ac - bs;
            y2[j] = bc + as;
        }
    }
    if (rp.interleaved) {
#pragma unroll
        for (int j = 0; j < 4; ++j) e0[2 * j] = y1[j], e0[2 * j + 1] = y2[j], e1[2 * j] = y1[4 + j], e1[2 * j + 1] = y2[4 + j];
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) e0[j] = y1[j], e1[j] = y2[j];
    }
    FASN_KVROPE_STORE(c1, kvrope_round<Tag>(e0));
    FASN_KVROPE_STORE(c2, kvrope_round<Tag>(e1));
#undef FASN_KVROPE_STORE
