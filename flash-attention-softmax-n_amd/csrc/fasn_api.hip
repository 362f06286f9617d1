// fasn_api.hip — the C ABI of libfasn (include/fasn.h): argument validation, parameter packing, dispatch.
// No allocation, no synchronisation, no environment variables: every exported symbol is declared in include/fasn.h.
#include <hip/hip_runtime.h>
#include <math.h>
#include <cxxabi.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "fasn.h"
#include "fasn_plan.h"
#include "fasn_bwd_launch.h"
#include "fasn_bwd_dn.h"

using namespace fasn;

namespace fasn {
thread_local LaunchLog* t_launch_log = nullptr;
// one line per launch: the kernel with its template arguments (demangled from the type name kernel_pretty_name<&kernel<...>> hands over:
// "fasn::KernelTag<&(void fasn::kernel<arguments>(fasn::Params))>"), grid, block, LDS
// "bf16,D=64,QB=2,plain,OCC=2,NW=4,RING=2,SEED=2" for "fasn_fwd_kernel<fasn::bf16_tag, 64, 2, 0, 2, 4, 0, 0, 2, 0, 2, 1, 0, 0>": the template
// arguments of the kernel families by NAME (flags that are off and unit factors are left out), so that a launch plan, a profile line or a
// spill table can be read without the kernel headers open. Unknown kernels: empty string.
static size_t describe_kernel(const char* name, size_t n, char* out, size_t cap) {
    struct Family { const char* base; const char* params; };   // params: names in template order; '!' prefix = omit when 0, '1' prefix = omit when 1, 'M' = mode, 'T' = element tag
    static const Family families[] = {
        {"fasn_fwd_kernel", "T D QB M OCC NW !PRIO !DROP RING !SPLIT SEED 1VH !FOLD !BF32"},
        {"fasn_bwd_dq_kernel", "T D QB M OCC !DROP DQ_SEED !BF32"},
        {"fasn_bwd_dkdv_kernel", "T D KB M OCC !DROP !GQA 1DH !BF32"},
        {"fasn_bwd_dq_ws_kernel", "T D M !DROP"},
        {"fasn_bwd_dkdv_ws_kernel", "T D M !GQA !DROP"},
        {"fasn_bwd_dq_pipe_kernel", "T M !DROP"},
        {"fasn_bwd_dkdv_pipe_kernel", "T M !DROP"},
        {"fasn_bwd_dq_ws256_kernel", "T M"},
        {"fasn_bwd_dkdv_ws256_kernel", "T M !GQA"},
        {"fasn_fwd_ws256_kernel", "T M !DROP"},
        {"fasn_bwd_delta_kernel", "T D"},
        {"fasn_fwd_combine_kernel", "T D"},
        {"fasn_bwd_dbias_ws_kernel", "T D"},
        {"fasn_bwd_dbias_kernel", "T D FAST"},
        {"fasn_f32_fwd_kernel", "D M"},
        {"fasn_f32_dq_kernel", "D M"},
        {"fasn_f32_dkdv_kernel", "D M"},
        {"fasn_f32_delta_kernel", "D"},
        {"fasn_kvcache_fwd_kernel", "T D"},
        {"fasn_kvcache_combine_kernel", "T D"},
        {"fasn_kvcache_append_kernel", "D"},
        {"fasn_kvprefill_fwd_kernel", "T D"},
        {"fasn_kvprefill_combine_kernel", "T D"},
        {"fasn_kvprefill_append_kernel", "D"},
        {"fasn_kvrope_kernel", "T D"},
        {"fasn_kvvarlen_schedule_kernel", "NT"},
        {"fasn_kvvarlen_fwd_kernel", "T D"},
        {"fasn_kvvarlen_combine_kernel", "T D"},
        {"fasn_kvvarlen_append_kernel", "D"},
        {"fasn_kvcache_fwd_fp8_kernel", "T D"},
        {"fasn_kvcache_fp8_combine_kernel", "T D"},
        {"fasn_kvcache_fp8_append_kernel", "T D"},
        {"fasn_kvprefill_fwd_fp8_kernel", "T D"},
        {"fasn_kvprefill_fp8_combine_kernel", "T D"},
        {"fasn_kvprefill_fp8_append_kernel", "T D"},
        {"fasn_kvcache_fwd_fp8_window_kernel", "T D"},
        {"fasn_kvprefill_fwd_fp8_window_kernel", "T D"},
        {"fasn_kvrope_fp8_kernel", "T D"},
        {"fasn_kvcache_fwd_fp8_tree_kernel", "T D"},
        {"fasn_kvprefill_fwd_fp8_tree_kernel", "T D"},
        {"fasn_kvrope_fp8_tree_kernel", "T D"},
        {"fasn_kvcache_fp8_tree_commit_kernel", "D"},
        {"fasn_varlen_tail_kernel", "TOK"},
        {"fasn_varlen_rope_kernel", "T D"},
    };
    static const char* const modes[] = {"plain", "causal", "bias+mask", "element-load", "bias", "mask", "keypad", "bias+keypad"};
    if (cap == 0) return 0;
    out[0] = 0;
    const char* lt = (const char*)memchr(name, '<', n);
    if (lt == nullptr) return 0;
    const Family* fam = nullptr;
    for (const Family& f : families)
        if (strlen(f.base) == (size_t)(lt - name) && strncmp(f.base, name, (size_t)(lt - name)) == 0) fam = &f;
    if (fam == nullptr) return 0;
    size_t len = 0;
    auto put = [&](const char* t, size_t tn) {
        if (len + tn + 1 < cap) {
            memcpy(out + len, t, tn);
            len += tn;
            out[len] = 0;
        }
    };
    const char* a = lt + 1;
    const char* pn = fam->params;
    const char* const end = name + n;
    while (a < end && *pn) {
        const char* ae = a;   // one template argument: up to the next ',' or the closing '>' (the arguments here are flat: types and integers)
        while (ae < end && *ae != ',' && *ae != '>') ++ae;
        const char* pe = pn;
        while (*pe && *pe != ' ') ++pe;
        while (a < ae && *a == ' ') ++a;
        char val[48];
        const size_t vn = (size_t)(ae - a) < sizeof val - 1 ? (size_t)(ae - a) : sizeof val - 1;
        memcpy(val, a, vn);
        val[vn] = 0;
        const long num = strtol(val, nullptr, 10);
        char item[96];
        int in = 0;
        if (*pn == 'T' && pe - pn == 1) in = snprintf(item, sizeof item, "%s%s", strstr(val, "bf16") ? "bf16" : "f16", strstr(val, "varlen") ? ",varlen" : "");   // (*_varlen_tag: packed variable-length items)
        else if (*pn == 'M' && pe - pn == 1) in = snprintf(item, sizeof item, "%s", (num >= 0 && num < 8) ? modes[num] : val);
        else if (*pn == '!') { if (strcmp(val, "0") != 0 && strcmp(val, "false") != 0) in = snprintf(item, sizeof item, "%.*s=%s", (int)(pe - pn - 1), pn + 1, val); }
        else if (*pn == '1') { if (num != 1) in = snprintf(item, sizeof item, "%.*s=%s", (int)(pe - pn - 1), pn + 1, val); }
        else in = snprintf(item, sizeof item, "%.*s=%s", (int)(pe - pn), pn, val);
        if (in > 0) {
            if (len) put(",", 1);
            put(item, (size_t)in);
        }
        a = ae < end ? ae + 1 : end;
        pn = *pe ? pe + 1 : pe;
    }
    return len;
}

void log_launch(const char* tag_name, unsigned grid, unsigned block, int smem) {
    LaunchLog* const g = t_launch_log;
    if (g == nullptr || g->buf == nullptr) return;   // (no buffer: the launch site has recorded the mode, and that is all such a log asks)
    int st = 0;
    char* dm = abi::__cxa_demangle(tag_name, nullptr, nullptr, &st);
    const char* b = dm ? strstr(dm, "&(void ") : nullptr;
    b = b ? b + 7 : (dm ? dm : tag_name);
    if (strncmp(b, "fasn::", 6) == 0) b += 6;
    if (strncmp(b, "(anonymous namespace)::", 23) == 0) b += 23;   // (fasn_moments.hip keeps its kernel file-local)
    size_t n = 0;
    for (int depth = 0; b[n] != 0; ++n) {   // the name ends at the parameter list: the first '(' outside the template arguments
        if (b[n] == '<') ++depth;
        else if (b[n] == '>') --depth;
        else if (b[n] == '(' && depth == 0) break;
    }
    char cfg[192];
    describe_kernel(b, n, cfg, sizeof cfg);
    char tail[320];
    const int tn = snprintf(tail, sizeof tail, " grid=%u block=%u lds=%d cfg=%s\n", grid, block, smem, cfg[0] ? cfg : "-");
    if (g->len + n + (size_t)tn + 1 > g->cap) {   // does not fit: remember that by moving len past cap (the caller reports FASN_EINVAL)
        g->len = g->cap + 1;
    } else {
        memcpy(g->buf + g->len, b, n);
        memcpy(g->buf + g->len + n, tail, (size_t)tn);
        g->len += n + (size_t)tn;
        g->buf[g->len] = 0;
    }
    free(dm);
}
int launch_fwd_f32(const FwdParams& p, const FwdLaunch& l, hipStream_t s);
int launch_bwd_f32(const BwdParams& p, const FwdLaunch& l, hipStream_t s);
}  // namespace fasn

namespace {

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// rows must stay 16-byte aligned: base pointer and every non-feature stride (in 2-byte elements) % 8
int check_view(const fasn_view4& v, bool required, int esize = 2) {
    if (v.ptr == nullptr) return required ? FASN_EINVAL : FASN_OK;
    if (v.stride[3] != 1) return FASN_ESTRIDE;
    if (!aligned16(v.ptr)) return FASN_EALIGN;
    for (int i = 0; i < 3; ++i)
        if (v.stride[i] % (16 / esize) != 0) return FASN_EALIGN;
    return FASN_OK;
}

// fp32 bias next to 16-bit q / k / v on the vector path (round 5): the head dims whose kernels have the fp32 image instantiation, forward and
// backward alike (head dims 32 / 64: the usual tuning points; head dim 128: the 8-wave forward with the register-staged two-buffer ring,
// fasn_fwd_d128.hip, and the ONE-wave backward kernels - the two-wave backward kernels have no LDS left for 8 KiB images; head dim 256: element
// loads). bias_vec only says that the BIAS is vector-movable: a call whose mode ends up MODE_GENERAL_SLOW for another reason (unaligned dense
// mask, fp16 scale overflow) still takes the element-load kernels, forward (launch_gen) and backward (launch_bwd_mode).
bool f32_bias_vector(int D) { return D == 32 || D == 64 || D == 128; }

int build_fwd(const fasn_fwd_args* a, FwdParams& p, FwdLaunch& l) {
    if (a == nullptr) return FASN_EINVAL;
    if (a->B <= 0 || a->H <= 0 || a->Sq <= 0 || a->Sk <= 0 || a->D <= 0 || a->Dv <= 0) return FASN_EINVAL;
    if (a->dtype != FASN_DTYPE_F16 && a->dtype != FASN_DTYPE_BF16 && a->dtype != FASN_DTYPE_F32) return FASN_EDTYPE;
    if (!fasn_supported(a->dtype, a->D, a->Dv)) return FASN_EHEADDIM;
    const int esize = a->dtype == FASN_DTYPE_F32 ? 4 : 2;
    // fp32 q/k/v: the bias, if any, must be fp32 as well (FASN_BIAS_SAME means fp32 then)
    if (!(a->dropout_p >= 0.f) || a->dropout_p >= 1.f) return FASN_EINVAL;
    if (!(a->softmax_n >= 0.f) || !(a->scale >= 0.f) || !isfinite(a->scale)) return FASN_EINVAL;
    int rc;
    if ((rc = check_view(a->q, true, esize))) return rc;
    if ((rc = check_view(a->k, true, esize))) return rc;
    if ((rc = check_view(a->v, true, esize))) return rc;
    if ((rc = check_view(a->o, true, esize))) return rc;
    if (a->bias.ptr != nullptr && a->bias_dtype != FASN_BIAS_SAME && a->bias_dtype != FASN_BIAS_F32) return FASN_EINVAL;

    p.q = (const char*)a->q.ptr;
    p.k = (const char*)a->k.ptr;
    p.v = (const char*)a->v.ptr;
    p.o = (char*)a->o.ptr;
    p.lse = a->lse;
    p.mask = (const uint8_t*)a->mask.ptr;
    p.bias = (const char*)a->bias.ptr;
    for (int i = 0; i < 3; ++i) {
        p.qs[i] = a->q.stride[i];
        p.ks[i] = a->k.stride[i];
        p.vs[i] = a->v.stride[i];
        p.os[i] = a->o.stride[i];
    }
    for (int i = 0; i < 4; ++i) {
        p.ms[i] = a->mask.ptr ? a->mask.stride[i] : 0;
        p.bs[i] = a->bias.ptr ? a->bias.stride[i] : 0;
    }
    p.B = a->B;
    p.H = a->H;
    p.Sq = a->Sq;
    p.Sk = a->Sk;
    p.nqblk = 0;
    p.causal = a->causal ? 1 : 0;
    p.bias_f32 = (a->bias.ptr && (a->bias_dtype == FASN_BIAS_F32 || esize == 4)) ? 1 : 0;
    p.bias_vec = 0;
    p.mask_vec = 0;
    p.keypad_fallback = 0;
    if (a->kv_group < 0 || (a->kv_group > 1 && a->H % a->kv_group != 0)) return FASN_EINVAL;
    p.kvg = a->kv_group > 1 ? a->kv_group : 1;
    p.batch_inner = 0;
    if (a->bias.ptr) {
        const int esz = p.bias_f32 ? 4 : 2;
        const int al = 4 * esz;  // 4 keys per load
        bool ok = a->bias.stride[3] == 1 && (reinterpret_cast<uintptr_t>(a->bias.ptr) % al) == 0;
        for (int i = 0; i < 3; ++i) ok = ok && ((a->bias.stride[i] * esz) % al == 0);
        // scale 0 takes the element-load path; so does an fp32 bias next to 16-bit q / k / v unless this head dim has the fp32 image
        // instantiation (no dropout, no split-K there), and any bias next to fp32 q / k / v (their kernels have the element-load mode only)
        const bool f32_ok = !p.bias_f32 || (esize == 2 && !(a->dropout_p > 0.f) && f32_bias_vector(a->D));
        p.bias_vec = (ok && f32_ok && a->scale > 0.f) ? 1 : 0;
    }
    if (a->mask.ptr) {
        bool ok = a->mask.stride[3] == 1 && (reinterpret_cast<uintptr_t>(a->mask.ptr) % 4) == 0;
        for (int i = 0; i < 3; ++i) ok = ok && (a->mask.stride[i] % 4 == 0);
        p.mask_vec = ok ? 1 : 0;
    }
    if (a->bias.ptr && a->bias.stride[0] == 0 && a->B > 1) p.batch_inner = 1;
    p.bias_bytes = p.mask_bytes = 0;
    {   // per-(b,h) slice extents for the buffer descriptors of the vector path; slices of 2 GiB or more use the element path
        const int64_t bb = a->bias.ptr ? ((int64_t)(a->Sq - 1) * a->bias.stride[2] + a->Sk) * (p.bias_f32 ? 4 : 2) : 0;
        const int64_t mb = a->mask.ptr ? ((int64_t)(a->Sq - 1) * a->mask.stride[2] + a->Sk) : 0;
        if (bb >= (1ll << 31)) p.bias_vec = 0;
        if (mb >= (1ll << 31)) p.mask_vec = 0;
        // the range check works on whole dwords: round the extent up so an odd tail (Sk % 2 for bias, Sk % 4 for mask) is
        // still fetched; the pointer is dword aligned, so the extra bytes share a dword with valid ones and are never used
        p.bias_bytes = (unsigned)((bb + 3) & ~3ll);
        p.mask_bytes = (unsigned)((mb + 3) & ~3ll);
    }
    // dropout: 16-bit threshold, drop probability thr/65536 (the nearest representable value to dropout_p, at least 1/65536)
    p.drop_thr = 0;
    p.drop_scale = 1.f;
    if (a->dropout_p > 0.f) {
        long thr = lrintf(a->dropout_p * 65536.f);
        thr = thr < 1 ? 1 : (thr > 65535 ? 65535 : thr);
        p.drop_thr = (unsigned)thr;
        p.drop_scale = 65536.f / (65536.f - (float)thr);
    }
    p.seed_lo = (unsigned)(a->seed & 0xffffffffu) ^ ((unsigned)a->offset * 0x9E3779B1u);
    p.seed_hi = (unsigned)(a->seed >> 32) + (unsigned)(a->offset >> 32);
    p.rng = a->rng_state;   // device {seed, offset}: overrides the two by-value words when given
    if (a->rng_state != nullptr && reinterpret_cast<uintptr_t>(a->rng_state) % 8) return FASN_EALIGN;
    p.c = a->scale * kLog2e;
    {
        // extent of one (b,h) matrix = last row start + one row (a length-1 sequence may carry stride 0)
        const int64_t kb = ((int64_t)(a->Sk - 1) * a->k.stride[2] + a->D) * esize, vb = ((int64_t)(a->Sk - 1) * a->v.stride[2] + a->Dv) * esize;
        if (kb <= 0 || vb <= 0 || kb >= (1ll << 31) || vb >= (1ll << 31)) return FASN_EINVAL;  // one (b,h) K/V matrix must span < 2 GiB
        p.kbytes = (unsigned)kb;
        p.vbytes = (unsigned)vb;
    }
    p.n = a->softmax_n;
    p.nt = nullptr;   // per-(batch, head) n: set by fasn_fwd_n only
    p.nsb = p.nsh = 0;

    l.dtype = a->dtype;
    l.D = a->D;
    if (a->mask.ptr || a->bias.ptr) {
        const bool vec = (!a->bias.ptr || p.bias_vec) && (!a->mask.ptr || p.mask_vec);
        l.mode = !vec ? MODE_GENERAL_SLOW : (a->bias.ptr && a->mask.ptr) ? MODE_GENERAL : a->bias.ptr ? MODE_GENERAL_B : MODE_GENERAL_M;
        // key-padding mask (one byte per key for the whole (b,h), no bias): plain kernels + a per-tile visibility word
        const bool kp_fits = (a->Sk + KT - 1) / KT <= kFwdKpMaxTiles;   // the forward kernels keep one visibility word per tile in LDS
        if (a->mask.ptr && !a->bias.ptr && a->mask.stride[2] == 0 && a->mask.stride[3] == 1 && kp_fits) {
            p.keypad_fallback = l.mode;   // what split-K and the fp32 kernels use: they have no key-padding path of their own
            l.mode = MODE_KEYPAD;
        } else if (a->mask.ptr && a->bias.ptr && p.bias_vec && a->mask.stride[2] == 0 && a->mask.stride[3] == 1 && a->dtype != FASN_DTYPE_F32 && kp_fits) {
            // vector bias + key-padding mask (ALiBi on a padded batch): bias through the vector path, mask as visibility bits
            p.keypad_fallback = l.mode;   // dropout and split-K instantiations take the dense-mask general mode instead
            l.mode = MODE_BIAS_KEYPAD;
        }
    } else {
        l.mode = a->causal ? MODE_CAUSAL : MODE_PLAIN;
    }
    // The vector kernels multiply Q (or K) by c = scale*log2e in the operand type before the MFMAs. In fp16 a large scale could
    // push an otherwise representable operand past 65504 there: such calls take the element-load kernels, which scale in fp32.
    if (a->dtype == FASN_DTYPE_F16 && fabsf(p.c) > 8.f) l.mode = MODE_GENERAL_SLOW;
    p.xq = nullptr;   // static deal of the items unless fasn_fwd_ws hands over counters (below)
    p.pair = 0;   // set per launch (paired causal blocks, fasn_launch.h)
    p.kprot = 1;
    p.nsplit = 1;
    p.tps = 0;
    p.part_o = nullptr;
    p.part_ml = nullptr;
    return FASN_OK;
}

// Split-K plan for short-query / long-key shapes: too few (b,h, query block) workgroups to fill 256 CUs while each one
// would walk many key tiles. Returns the number of key splits (1 = do not split) and the tiles per split (even).
int plan_splitk(const fasn_fwd_args* a, const FwdParams& p, const FwdLaunch& l, int& tps) {
    tps = 0;
    if (l.dtype == FASN_DTYPE_F32 || p.drop_thr || l.mode == MODE_GENERAL_SLOW || l.D > 128) return 1;
    if (p.bias_f32 && p.bias_vec) return 1;   // (the fp32 bias image has no split-K instantiation)
    if ((l.mode == MODE_KEYPAD || l.mode == MODE_BIAS_KEYPAD) && p.keypad_fallback == MODE_GENERAL_SLOW) return 1;
    const int64_t base_blocks = (int64_t)a->B * a->H * ((a->Sq + 127) / 128);
    int ntiles = (a->Sk + KT - 1) / KT;
    if (a->causal) {   // the last row's visible keys bound the walk
        const int kmax = a->Sk - 1;
        ntiles = kmax / KT + 1;
    }
    if (base_blocks >= 256 || ntiles < 16) return 1;
    int nsplit = (int)((1024 + base_blocks - 1) / base_blocks);
    if (nsplit > ntiles / 6) nsplit = ntiles / 6;
    if (nsplit < 2) return 1;
    tps = (ntiles + nsplit - 1) / nsplit;
    tps = (tps + 5) / 6 * 6;   // multiple of 6: the LDS buffer rotation (2 or 3 buffers) starts at buffer 0 in every split
    nsplit = (ntiles + tps - 1) / tps;
    return nsplit < 2 ? 1 : nsplit;
}
size_t splitk_bytes(const fasn_fwd_args* a, int nsplit) {
    return (size_t)a->B * a->H * nsplit * a->Sq * (size_t)(a->D + 2) * sizeof(float);
}

int dispatch_fwd(const FwdParams& p, const FwdLaunch& l, hipStream_t s) {
    if (l.dtype == FASN_DTYPE_F32) return launch_fwd_f32(p, l, s);
    switch (l.D) {
        case 32: return launch_fwd_d32(p, l, s);
        case 64: return launch_fwd_d64(p, l, s);
        case 128: return launch_fwd_d128(p, l, s);
        case 256: return launch_fwd_d256(p, l, s);
        default: return FASN_EHEADDIM;
    }
}

}  // namespace

namespace {
__global__ void rng_advance_kernel(uint64_t* state, uint64_t* out, uint64_t increment) {
    // fetch-add: two streams of one device advancing the same stream position concurrently never draw the same offset
    const uint64_t s = state[0];
    const uint64_t o = atomicAdd(reinterpret_cast<unsigned long long*>(state + 1), (unsigned long long)increment);
    if (out != nullptr) {
        out[0] = s;
        out[1] = o;
    }
}
}  // namespace

extern "C" {

int fasn_abi_version(void) { return FASN_ABI_VERSION; }

int fasn_rng_advance(uint64_t* state, uint64_t* out, uint64_t increment, fasn_stream_t stream) {
    if (state == nullptr || reinterpret_cast<uintptr_t>(state) % 8 || reinterpret_cast<uintptr_t>(out) % 8) return FASN_EINVAL;
    hipLaunchKernelGGL(rng_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state, out, increment);
    return hipGetLastError() == hipSuccess ? FASN_OK : FASN_ELAUNCH;
}

const char* fasn_strerror(int code) {
    switch (code) {
        case FASN_OK: return "ok";
        case FASN_EINVAL: return "invalid argument (null pointer, non-positive size, negative n/scale, bad enum)";
        case FASN_EDTYPE: return "unsupported element type (supported: fp16, bf16, fp32)";
        case FASN_EHEADDIM: return "unsupported head dimension (supported: D == Dv in {32, 64, 128}, and 256 for fp16 / bf16)";
        case FASN_EALIGN: return "pointer or stride breaks the 16-byte row alignment rule";
        case FASN_ESTRIDE: return "feature (last-dim) stride must be 1";
        case FASN_ELAUNCH: return "kernel launch failed";
        case FASN_EUNSUPPORTED: return "request not implemented in this build";
        case FASN_EWORKSPACE: return "workspace missing or too small";
        default: return "unknown fasn error";
    }
}

int fasn_supported(int32_t dtype, int32_t D, int32_t Dv) {
    if (dtype != FASN_DTYPE_F16 && dtype != FASN_DTYPE_BF16 && dtype != FASN_DTYPE_F32) return 0;
    if (D != Dv) return 0;
    if (D == 256) return dtype != FASN_DTYPE_F32 ? 1 : 0;   // 16-bit MFMA kernels only at this head dim
    return (D == 32 || D == 64 || D == 128) ? 1 : 0;
}

int fasn_fwd(const fasn_fwd_args* args, fasn_stream_t stream) {
    FwdParams p;
    FwdLaunch l;
    const int rc = build_fwd(args, p, l);
    if (rc) return rc;
    return dispatch_fwd(p, l, (hipStream_t)stream);
}

int fasn_fwd_path(const fasn_fwd_args* args) {
    FwdParams p;
    FwdLaunch l;
    const int rc = build_fwd(args, p, l);
    if (rc) return rc;
    if (l.dtype == FASN_DTYPE_F32) return FASN_PATH_FP32;
    // The family of the call's MODE, not of the kernel that serves it: a 16-bit bias alone at D = 128 runs the bias + key-padding kernel
    // with every key kept and is FASN_PATH_VECTOR all the same. D = 256 has modes it serves through others: the launcher's own rule.
    switch (l.D > 128 ? fwd_d256_mode(p, l.mode) : l.mode) {
        case MODE_PLAIN: case MODE_CAUSAL: return FASN_PATH_PLAIN;
        case MODE_KEYPAD: return FASN_PATH_KEYPAD;
        case MODE_BIAS_KEYPAD: return FASN_PATH_BIAS_KEYPAD;
        case MODE_GENERAL_SLOW: return FASN_PATH_ELEMENT;
        default: return FASN_PATH_VECTOR;
    }
}

// Long plain / causal launches at D = 64 deal their items dynamically across XCDs when the caller hands over 32 bytes of workspace for the eight
// counters (fasn_fwd_kernel.h: draw_item): from 8 rounds of workgroups (M0's four rounds lose 0.6 % to the memset and the atomics, 16 rounds gain 2 %).
static bool xq_wanted(const FwdParams& p, const FwdLaunch& l) {
    if (l.D != 64 || l.dtype == FASN_DTYPE_F32 || p.drop_thr || ((p.B * p.H) & 7) || p.Sq < 256) return false;
    const long blocks = (long)((p.Sq + 255) / 256) * p.B * p.H;
    if (l.mode == MODE_PLAIN) return blocks >= 8 * 512;
    if (l.mode == MODE_CAUSAL) return blocks >= 2 * 8 * 512;   // (paired blocks: half as many workgroups)
    return false;
}
constexpr size_t kXqBytes = 64;

size_t fasn_fwd_workspace_bytes(const fasn_fwd_args* args) {
    FwdParams p;
    FwdLaunch l;
    if (build_fwd(args, p, l)) return 0;
    int tps;
    const int nsplit = plan_splitk(args, p, l, tps);
    if (nsplit > 1) return splitk_bytes(args, nsplit);
    return xq_wanted(p, l) ? kXqBytes : 0;
}

// fasn_fwd_ws, and fasn_fwd_n with its per-(batch, head) n (nt != nullptr): the same plan, the kernels only read n elsewhere
static int fwd_ws(const fasn_fwd_args* args, void* workspace, size_t workspace_bytes, hipStream_t stream, const float* nt, int nsb, int nsh) {
    FwdParams p;
    FwdLaunch l;
    const int rc = build_fwd(args, p, l);
    if (rc) return rc;
    p.nt = nt;
    p.nsb = nsb;
    p.nsh = nsh;
    int tps;
    const int nsplit = plan_splitk(args, p, l, tps);
    if (nsplit > 1 && workspace != nullptr && workspace_bytes >= splitk_bytes(args, nsplit)) {
        if (reinterpret_cast<uintptr_t>(workspace) % 16) return FASN_EALIGN;
        p.nsplit = nsplit;
        p.tps = tps;
        p.part_o = static_cast<float*>(workspace);
        p.part_ml = p.part_o + (size_t)args->B * args->H * nsplit * args->Sq * args->D;
        return launch_fwd_splitk(p, l, stream);
    }
    if (nsplit <= 1 && workspace != nullptr && workspace_bytes >= kXqBytes && xq_wanted(p, l)) {
        if (reinterpret_cast<uintptr_t>(workspace) % 4) return FASN_EALIGN;
        p.xq = static_cast<int*>(workspace);
    }
    return dispatch_fwd(p, l, stream);
}

int fasn_fwd_ws(const fasn_fwd_args* args, void* workspace, size_t workspace_bytes, fasn_stream_t stream) {
    return fwd_ws(args, workspace, workspace_bytes, (hipStream_t)stream, nullptr, 0, 0);
}

int fasn_fwd_n(const fasn_fwd_args* args, const float* n, int64_t n_stride_b, int64_t n_stride_h, void* workspace, size_t workspace_bytes,
               fasn_stream_t stream) {
    if (n == nullptr) return fasn_fwd_ws(args, workspace, workspace_bytes, stream);
    if (args == nullptr) return FASN_EINVAL;
    if (reinterpret_cast<uintptr_t>(n) % 4) return FASN_EALIGN;
    // the kernels index n with 32-bit offsets: every (b, h) must address an element below 2^31
    if (n_stride_b < 0 || n_stride_h < 0 || (args->B > 0 && args->H > 0 &&
        (int64_t)(args->B - 1) * n_stride_b + (int64_t)(args->H - 1) * n_stride_h >= (1ll << 31)))
        return FASN_EINVAL;
    fasn_fwd_args a = *args;
    a.softmax_n = 0.f;   // ignored: the value check of the scalar does not apply
    return fwd_ws(&a, workspace, workspace_bytes, (hipStream_t)stream, n, (int)n_stride_b, (int)n_stride_h);
}

// The backward needs no workspace: FASN_BWD_ONE_PASS is accepted and ignored (the one-pass backward it once asked for was a measured loser on
// MI355X).
size_t fasn_bwd_workspace_bytes(const fasn_bwd_args* args) {
    (void)args;
    return 0;
}

int fasn_bwd(const fasn_bwd_args* a, fasn_stream_t stream) {
    if (a == nullptr) return FASN_EINVAL;
    FwdParams fp;
    FwdLaunch l;
    int rc = build_fwd(&a->fwd, fp, l);
    if (rc) return rc;
    if (a->fwd.lse == nullptr || a->delta == nullptr) return FASN_EINVAL;
    if (l.mode == MODE_KEYPAD && l.dtype == FASN_DTYPE_F32) l.mode = MODE_GENERAL_SLOW;   // (the fp32 kernels have the element-load mask path only)
    const int esize = a->fwd.dtype == FASN_DTYPE_F32 ? 4 : 2;
    if ((rc = check_view(a->dout, true, esize))) return rc;
    if ((rc = check_view(a->dq, true, esize))) return rc;
    if ((rc = check_view(a->dk, true, esize))) return rc;
    if ((rc = check_view(a->dv, true, esize))) return rc;
    BwdParams p;
    p.f = fp;
    p.dout = (const char*)a->dout.ptr;
    p.dq = (char*)a->dq.ptr;
    p.dk = (char*)a->dk.ptr;
    p.dv = (char*)a->dv.ptr;
    p.delta = a->delta;
    p.scale = a->fwd.scale;
    {
        const int64_t qb = ((int64_t)(a->fwd.Sq - 1) * a->fwd.q.stride[2] + a->fwd.D) * esize;
        const int64_t db = ((int64_t)(a->fwd.Sq - 1) * a->dout.stride[2] + a->fwd.Dv) * esize;
        if (qb <= 0 || db <= 0 || qb >= (1ll << 31) || db >= (1ll << 31)) return FASN_EINVAL;
        p.qbytes = (unsigned)qb;
        p.dobytes = (unsigned)db;
    }
    p.dqacc = nullptr;   // unused
    p.skip = 0;
    p.dbias = nullptr;
    p.dbias_vec = 0;
    for (int i = 0; i < 3; ++i) p.dbs[i] = 0;
    bool dbias_reduced = false;
    int dbias_f32 = 0;
    if (a->dbias.ptr != nullptr) {
        if (a->fwd.bias.ptr == nullptr) return FASN_EINVAL;   // nothing to differentiate
        if (a->dbias.stride[3] != 1) return FASN_ESTRIDE;
        // reduced form: the gradient summed over a broadcast batch and / or head dimension by the dbias kernel
        dbias_reduced = (a->dbias.stride[0] == 0 && a->fwd.B > 1) || (a->dbias.stride[1] == 0 && a->fwd.H > 1);
        if (dbias_reduced && (l.dtype == FASN_DTYPE_F32 || fp.drop_thr != 0 || a->dbias.stride[2] == 0)) return FASN_EUNSUPPORTED;
        dbias_f32 = (dbias_reduced && a->dbias_dtype == FASN_BIAS_F32) ? 1 : 0;
        const int osz = dbias_f32 ? 4 : esize;
        if (reinterpret_cast<uintptr_t>(a->dbias.ptr) % osz) return FASN_EALIGN;
        p.dbias = (char*)a->dbias.ptr;
        bool vec = reinterpret_cast<uintptr_t>(a->dbias.ptr) % 16 == 0;
        for (int i = 0; i < 3; ++i) {
            p.dbs[i] = a->dbias.stride[i];
            vec = vec && (a->dbias.stride[i] * osz) % 16 == 0;
        }
        p.dbias_vec = vec ? 1 : 0;
    }
    for (int i = 0; i < 3; ++i) {
        p.dos[i] = a->dout.stride[i];
        p.dqs[i] = a->dq.stride[i];
        p.dks[i] = a->dk.stride[i];
        p.dvs[i] = a->dv.stride[i];
    }
    if (l.dtype == FASN_DTYPE_F32) return launch_bwd_f32(p, l, (hipStream_t)stream);
    if (dbias_reduced) {   // dQ / dK / dV without the dense dS store, then the bias gradient by its own kernel (it needs delta)
        BwdParams pg = p;
        pg.dbias = nullptr;
        const int rc2 = launch_bwd(pg, l, (hipStream_t)stream);
        if (rc2) return rc2;
        return launch_bwd_dbias(p, l, a->dbias.stride[0] == 0 ? 1 : a->fwd.B, a->dbias.stride[1] == 0 ? 1 : a->fwd.H, dbias_f32, (hipStream_t)stream);
    }
    return launch_bwd(p, l, (hipStream_t)stream);
}

// dn: the stage-1 plan of fasn_bwd_dn (rows per workgroup from the row size of O); FASN_OK or the FASN_E* code of the call
static int bwd_dn_plan(const fasn_bwd_args* a, DnParams& d) {
    if (a == nullptr) return FASN_EINVAL;
    fasn_fwd_args f = a->fwd;
    f.softmax_n = 0.f;   // (a forward through fasn_fwd_n ignored the scalar; so does its gradient)
    FwdParams fp;
    FwdLaunch l;
    int rc = build_fwd(&f, fp, l);
    if (rc) return rc;
    if (f.lse == nullptr) return FASN_EINVAL;
    const int esize = f.dtype == FASN_DTYPE_F32 ? 4 : 2;
    if ((rc = check_view(a->dout, true, esize))) return rc;
    d.o = (const char*)f.o.ptr;
    d.dout = (const char*)a->dout.ptr;
    d.lse = f.lse;
    for (int i = 0; i < 3; ++i) {
        d.os[i] = f.o.stride[i];
        d.dos[i] = a->dout.stride[i];
    }
    d.B = f.B;
    d.H = f.H;
    d.Sq = f.Sq;
    d.cpr = f.Dv * esize / 16;   // 4 .. 32 for the supported head dims
    d.rpw = dn_rows_per_workgroup(d.cpr);
    d.nchunk = (f.Sq + d.rpw - 1) / d.rpw;
    return FASN_OK;
}

size_t fasn_bwd_dn_workspace_bytes(const fasn_bwd_args* args) {
    DnParams d;
    if (bwd_dn_plan(args, d)) return 0;
    return (size_t)d.B * d.H * d.nchunk * sizeof(float);
}

int fasn_bwd_dn(const fasn_bwd_args* args, float* dn, int64_t dn_stride_b, int64_t dn_stride_h, void* workspace, size_t workspace_bytes,
                fasn_stream_t stream) {
    DnParams d;
    const int rc = bwd_dn_plan(args, d);
    if (rc) return rc;
    if (dn == nullptr || dn_stride_b < 0 || dn_stride_h < 0) return FASN_EINVAL;
    if (reinterpret_cast<uintptr_t>(dn) % 4) return FASN_EALIGN;
    if (workspace == nullptr || workspace_bytes < (size_t)d.B * d.H * d.nchunk * sizeof(float)) return FASN_EWORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) % 16) return FASN_EALIGN;
    d.part = static_cast<float*>(workspace);
    d.dn = dn;
    d.dsb = dn_stride_b;
    d.dsh = dn_stride_h;
    d.Bo = dn_stride_b == 0 ? 1 : d.B;   // a zero stride: the sum over that dimension
    d.Ho = dn_stride_h == 0 ? 1 : d.H;
    return launch_bwd_dn(d, args->fwd.dtype, (hipStream_t)stream);
}

int fasn_launch_plan(const fasn_bwd_args* args, int32_t which, char* buf, size_t cap) {
    if (args == nullptr || which < FASN_PLAN_FWD || which > FASN_PLAN_FWD_WS) return FASN_EINVAL;
    return record_plan(buf, cap, [&] {
        if (which == FASN_PLAN_FWD) return fasn_fwd(&args->fwd, nullptr);
        if (which == FASN_PLAN_BWD) return fasn_bwd(args, nullptr);
        return fasn_fwd_ws(&args->fwd, plan_workspace(), ~size_t(0), nullptr);
    });
}

// The family the BACKWARD of a call is routed to: the forward's, or FASN_PATH_ELEMENT when the backward's own launch record (LaunchLog::modes
// of the call under the recorder, no text) holds an element-load instantiation - asked of the launch tables themselves, so it cannot drift
// from them. Differs from fasn_fwd_path at head dim 256, where masks other than key padding and every bias have vector kernels in the
// forward only.
int fasn_bwd_path(const fasn_bwd_args* args) {
    if (args == nullptr) return FASN_EINVAL;
    const int fp = fasn_fwd_path(&args->fwd);
    if (fp < 0 || fp == FASN_PATH_FP32 || fp == FASN_PATH_ELEMENT) return fp;
    LaunchLog log{};
    const int rc = record_plan(log, [&] { return fasn_bwd(args, nullptr); });
    if (rc < 0) return rc;
    return (log.modes & (1u << MODE_GENERAL_SLOW)) ? FASN_PATH_ELEMENT : fp;
}

}  // extern "C"
