// fasn_mla_tile.inc — one 64-key tile of the MLA decode walk, for a wave that has rows: S^T over the 576 features, the mask, the online
// softmax in the lane, O^T over the wave's 256 value features. Included by fasn_mla_fwd_kernel (fasn_mla.h) and by its sibling over an FP8
// cache (fasn_mla_fp8.h), which differ in where the 16-bit tile image lies and in the factor on the scores:
//   MLA_TILE_AT    byte offset of this tile's image behind the lane parts ka / va
//   MLA_SCORE(x)   the fp32 score x of the MFMAs in the log2 domain
// and, with the kernel over an index list (fasn_mla_sparse.h), in what a visible key is (k0 = t * 64 is this tile's first key of a walk):
//   MLA_TILE_ALL_VISIBLE     every row sees every key of the tile (wave-uniform)
//   MLA_KEY_VISIBLE(kb, r)   the lane's row sees the key of accumulator register r of key block kb: key kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi
// Everything else - t, the lane parts, qf, the row's (m_run, l_run) and oacc - is the including kernel's.
{
    // the lane parts inside this tile's buffer, opaque so that the literals stay literals (the instructions' offset fields)
    uint32_t kt[4], vt[2][2];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        kt[j] = ka[j] + MLA_TILE_AT;
        asm volatile("" : "+v"(kt[j]));
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        vt[j >> 1][j & 1] = va[j >> 1][j & 1] + MLA_TILE_AT;
        asm volatile("" : "+v"(vt[j >> 1][j & 1]));
    }
    const int k0 = t * KV_KT;
    f32x16 sacc[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
        for (int r = 0; r < 16; ++r) sacc[kb][r] = 0.f;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const vec8 kf = mla_lds_read16<vec8>(kt[s & 3] + (kb * 32 * MLA_ROWB + (s >> 2) * 128));
            sacc[kb] = E::mfma(kf, qf[s], sacc[kb]);
        }
    }
    // hidden keys (beyond the row's causal limit, which is below len_b) at -inf
    float mx = -INFINITY;
    if (MLA_TILE_ALL_VISIBLE) {   // wave-uniform (lanes without a row carry zero queries; their state is never stored)
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                sacc[kb][r] = MLA_SCORE(sacc[kb][r]);
                mx = fmaxf(mx, sacc[kb][r]);
            }
    } else {
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float y = MLA_KEY_VISIBLE(kb, r) ? MLA_SCORE(sacc[kb][r]) : -INFINITY;
                sacc[kb][r] = y;
                mx = fmaxf(mx, y);
            }
    }
    mx = max_across_halves(mx);
    const float m_new = fmaxf(m_run, mx);
    const float m_use = (m_new == -INFINITY) ? 0.f : m_new;   // nothing visible so far
    const float alpha = fast_exp2(m_run - m_use);
    float rs = 0.f;
    vec8 pf[2][2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2) {
            f32x8 x;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                x[e] = fast_exp2(sacc[kb][8 * t2 + e] - m_use);
                rs += x[e];
            }
            pf[kb][t2] = E::cvt8(x);
        }
    l_run = l_run * alpha + rs;
    m_run = m_new;
    if (!__all(alpha == 1.0f)) {
#pragma unroll
        for (int d = 0; d < DBW; ++d)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[d][r] *= alpha;
    }
    // O^T += V^T P^T over the wave's 8 feature blocks of the latent: the same image, read along the keys
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
            for (int d = 0; d < DBW; ++d) {
                const int lit = (kb * 32 + 16 * t2) * MLA_ROWB + (d >> 1) * 128;
                const vec8 vf = mla_lds_read_tr<vec8>(vt[d & 1][0] + lit, vt[d & 1][1] + lit);
                oacc[d] = E::mfma(vf, pf[kb][t2], oacc[d]);
            }
}
