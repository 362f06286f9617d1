/*
 * fasn.h — C ABI of libfasn: fused attention with softmax_n for AMD MI355X (gfx950 / CDNA4).
 *
 *   softmax_n(x)_i = exp(x_i) / (n + sum_j exp(x_j)),   real n >= 0
 *   O = softmax_n(scale * Q K^T + bias  [masked / causal -> -inf]) V
 *
 * This is the drop-in boundary for the reference's kernel-launch sites:
 *   - flash_attention_softmax_n/core/flash_attn.py:115-124   (torch SDPA call on zero-row-padded K/V)
 *   - flash_attention_softmax_n/core/flash_attn_triton.py:278-291  (_fwd_kernel launch)
 *   - flash_attention_softmax_n/core/flash_attn_triton.py:316-335  (_bwd_preprocess + _bwd_kernel launches)
 * Host code (Python, PyTorch-ROCm) normalises arguments and calls these entry points through ctypes;
 * see INTEGRATION.md for the reference-side binding.
 *
 * Contract
 *   - plain C, no torch types: device pointers, element strides, sizes.
 *   - the library never allocates, frees or synchronises; every buffer (incl. workspace) is caller-owned.
 *   - launches are asynchronous on the hipStream_t passed in (0 = default stream).
 *   - stateless and re-entrant; the current HIP device must be the one owning the pointers.
 *   - returns FASN_OK (0) or a negative FASN_E* code; never throws, never aborts.
 *
 * Tensor layout: 4-D (batch, head, seq, feature) addressed by element strides; the feature stride
 * must be 1 and base pointers / other strides must keep every row 16-byte aligned (strides % 8 elements for the 16-bit
 * types, % 4 for fp32). A stride of 0 is
 * a broadcast dimension (mask, bias, and the head dimension of K/V for shared-KV layouts). The rule holds for the inputs (q, k, v,
 * dout, mask, bias) and for the outputs (o, dq, dk, dv, dbias) alike: each is addressed by its own strides, none has to be contiguous,
 * and no two have to share a layout; batch and head strides are 64-bit and unbounded. lse and delta are contiguous [B, H, Sq].
 *
 * The span rule. The span of one (batch, head) matrix of an operand with `rows` rows of `width` elements is
 * ((rows - 1) * row_stride + width) * element_size bytes - the last row's start plus one row. The vector kernels address such a matrix
 * through a 32-bit buffer descriptor, so:
 *   - K and V (rows = Sk): a span of 2^31 bytes or more is FASN_EINVAL in every call that takes a fasn_fwd_args (fasn_fwd, fasn_fwd_ws,
 *     fasn_fwd_n, fasn_bwd, fasn_bwd_dn, the workspace and path queries).
 *   - Q and dout (rows = Sq): a span of 2^31 bytes or more is FASN_EINVAL in fasn_bwd only. The forward reads Q by 64-bit addresses and
 *     has no such bound - a call may therefore pass fasn_fwd and be refused by fasn_bwd; a caller that differentiates copies such a Q
 *     (or dout) into a denser buffer first (flash_attn._canon does).
 *   - mask and bias (rows = Sq, width = Sk): a span of 2^31 bytes or more is no error; the call takes the element-load kernels
 *     (FASN_PATH_ELEMENT), which address every element in 64 bits.
 *   - o, dq, dk, dv, dbias: written through 64-bit addresses, no bound.
 * With a 16-bit type and 65 rows the largest legal row stride is therefore (2^31 - 2 width) / 128 elements rounded down to a
 * multiple of 8; the kernels' 32-bit tile and lane offsets (rows * row_stride * element_size) are sized for exactly that bound.
 */
#ifndef FASN_H_
#define FASN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FASN_ABI_VERSION 6

/* error codes */
#define FASN_OK 0
#define FASN_EINVAL (-1)      /* NULL pointer / non-positive size / bad enum */
#define FASN_EDTYPE (-2)      /* unsupported element type */
#define FASN_EHEADDIM (-3)    /* unsupported head dimension (supported: 32, 64, 128 and - fp16 / bf16 - 256; D == Dv) */
#define FASN_EALIGN (-4)      /* pointer or stride breaks the 16-byte row alignment rule */
#define FASN_ESTRIDE (-5)     /* feature stride != 1 */
#define FASN_ELAUNCH (-6)     /* hipLaunchKernel / hipGetLastError failure */
#define FASN_EUNSUPPORTED (-7)/* valid request this build does not implement (e.g. a reduced bias gradient with fp32 q/k/v or dropout) */
#define FASN_EWORKSPACE (-8)  /* workspace missing or too small */

/* element types of q/k/v/o/do/dq/dk/dv (FASN_DTYPE_F32 = 2, defined below: exact-fp32 MFMA kernels; with fp32 q/k/v the
   bias, if any, is fp32 too and mask / bias / dropout take an element-load instantiation) */
#define FASN_DTYPE_F16 0
#define FASN_DTYPE_BF16 1

/* element type of the additive bias */
#define FASN_BIAS_NONE 0
#define FASN_BIAS_SAME 1 /* same dtype as q */
#define FASN_BIAS_F32 2

typedef void* fasn_stream_t; /* hipStream_t */

/* One 4-D tensor view: ptr + element strides for (batch, head, row, col). */
typedef struct fasn_view4 {
    void* ptr;
    int64_t stride[4];
} fasn_view4;

/*
 * Forward. Replaces: _fwd_kernel launch (flash_attn_triton.py:278-291) and the SDPA call
 * (flash_attn.py:117-124) including its K/V zero-row padding (:66-73) and dense mask
 * materialisation (:87-113), which are expressed here as `softmax_n`, `causal`, `mask`, `bias`.
 */
typedef struct fasn_fwd_args {
    fasn_view4 q;   /* [B,H,Sq,D]  */
    fasn_view4 k;   /* [B,H,Sk,D]  */
    fasn_view4 v;   /* [B,H,Sk,Dv] */
    fasn_view4 o;   /* [B,H,Sq,Dv] out */
    float* lse;     /* [B,H,Sq] fp32 contiguous, out: log(n + sum_j exp(x_ij)) (natural log); may be NULL */
    fasn_view4 mask;/* optional, uint8/bool, nonzero = attend; strides may be 0; ptr NULL = none */
    fasn_view4 bias;/* optional additive bias (added after scaling); ptr NULL = none */
    int32_t bias_dtype; /* FASN_BIAS_* */
    int32_t dtype;      /* FASN_DTYPE_* */
    int32_t B, H, Sq, Sk, D, Dv;
    float scale;        /* multiplies q.k before bias (reference default 1/sqrt(D)) */
    float softmax_n;    /* n >= 0, real-valued */
    int32_t causal;     /* bottom-right aligned: key j visible to row i iff j <= i + Sk - Sq */
    float dropout_p;    /* in [0,1): attention-weight dropout; realised as thr/65536 with thr = round(65536 p) in [1,65535] */
    uint64_t seed, offset; /* dropout stream: the keep bit of (b,h,row,key) is a pure function of (seed, offset, indices);
                              pass the SAME values to fasn_bwd (see flash-attention-softmax-n_amd/dropout.py). The function is part
                              of FASN_ABI_VERSION - it changed in ABI 6 - so a mask is reproducible within one ABI version only */
    int32_t kv_group;      /* grouped-query attention (ABI 2): query head h reads K/V head h / kv_group, i.e. k and v are
                              [B, H / kv_group, Sk, D] addressed through their head stride; 0 or 1 = one K/V head per query
                              head. fasn_bwd writes dk / dv per K/V head, [B, H / kv_group, Sk, D]: each dK/dV workgroup walks the
                              query heads of its group and accumulates their contributions in registers (fp32). */
    const uint64_t* rng_state; /* optional (ABI 3): DEVICE pointer to {seed, offset} (8-byte aligned). When set, the kernels read the
                              dropout stream position from device memory instead of `seed` / `offset` above, so a captured HIP graph
                              that also captures fasn_rng_advance() draws a fresh mask on every replay. Pass the same pointer (and the
                              same contents) to fasn_bwd. NULL = use the by-value fields. */
} fasn_fwd_args;

/*
 * Backward. Replaces _bwd_preprocess + _bwd_kernel (flash_attn_triton.py:316-335), with the
 * softmax_n-correct LSE (the reference's Triton backward drops n).
 * dq/dk/dv are written (not accumulated) in `dtype`. `delta` is a [B,H,Sq] fp32 scratch the
 * caller provides.
 *
 * Plan: a dQ kernel and a dK/dV kernel that each recompute S and dP (7 GEMMs for the 5 of the algorithm, deterministic, no
 * workspace). The single 5-GEMM kernel of the reference (flash_attn_triton.py:199-226; dQ by load-add-store, here fp32 atomics
 * into a caller-provided accumulator) was built in round 3 and measured slower on MI355X in every form:
 * it is no longer part of the sources. The library ignores FASN_BWD_ONE_PASS, fasn_bwd_workspace_bytes() returns 0
 * and `workspace` may be NULL; the fields stay in the struct so that the ABI version does not change.
 */
#define FASN_BWD_ONE_PASS 1 /* fasn_bwd_args.flags: reserved (the one-pass backward, no longer built); ignored by libfasn.so */
typedef struct fasn_bwd_args {
    fasn_fwd_args fwd; /* same views as forward; o and lse are inputs here. A row with lse = -inf or lse < -2^22 (a row that saw only
                          keys under an additive mask such as -1e9, and no sink) has no weights: it adds 0 to every gradient */
    fasn_view4 dout;   /* [B,H,Sq,Dv] */
    fasn_view4 dq;     /* [B,H,Sq,D]  out */
    fasn_view4 dk;     /* [B,H/kv_group,Sk,D]  out (summed over the query heads of a GQA group inside the kernel) */
    fasn_view4 dv;     /* [B,H/kv_group,Sk,Dv] out */
    float* delta;      /* [B,H,Sq] fp32 scratch */
    void* workspace;
    size_t workspace_bytes;
    fasn_view4 dbias;  /* optional out (ABI 2): gradient of the additive bias, key stride 1; ptr NULL = not wanted. Needs fwd.bias.
                          Dense form: dS as [B,H,Sq,Sk] in `dtype` (the dQ kernels store it; the caller sums over whatever its
                          bias broadcasts). Reduced form (ABI 4): a batch and / or head stride of 0 (with B > 1 / H > 1) asks for the
                          sum over that dimension - dbias is then [1 or B, 1 or H, Sq, Sk], written once by a kernel that walks
                          the (b,h) sharing each bias tile (csrc/fasn_bwd_dbias_ws.h / fasn_bwd_dbias.h; 16-bit q/k/v, no dropout; no [B,H,Sq,Sk]
                          buffer anywhere). */
    int32_t flags;     /* ABI 4: FASN_BWD_* bits, 0 = default */
    int32_t dbias_dtype; /* ABI 4, reduced form only: FASN_BIAS_SAME (0 means the same) = `dtype`, FASN_BIAS_F32 = fp32 elements */
} fasn_bwd_args;

int fasn_abi_version(void);
const char* fasn_strerror(int code);

/* 1 if (dtype, D, Dv) has a compiled kernel, else 0. */
int fasn_supported(int32_t dtype, int32_t D, int32_t Dv);

int fasn_fwd(const fasn_fwd_args* args, fasn_stream_t stream);

/*
 * Which kernel family `args` is routed to (ABI 4; the backward: fasn_bwd_path below - the same family except at head dim 256): a non-negative
 * FASN_PATH_* value, or a negative FASN_E* code for arguments fasn_fwd would refuse. Every family gives the same results; they
 * differ in speed. FASN_PATH_ELEMENT is the one to know about: masks / biases whose rows cannot be moved in aligned vector
 * pieces (unaligned or strided rows, key stride != 1; an fp32 bias next to 16-bit q at head dim 256, under dropout, or with rows
 * that are not 16-byte aligned - at head dims <= 128 an aligned fp32 bias takes the vector family since ABI 5), scale <= 0 with a bias, fp16 with
 * scale*log2(e) > 8 take per-element loads and run 3-5 x slower than the vector path. Nothing is launched. (The reference has no
 * counterpart: its SDPA backends are picked inside torch.)
 * The value names the family of the call's operands, except at head dim 256 UNDER DROPOUT (ABI 6), where one vector instantiation serves
 * every call whose mask / bias rows move as vectors: such a call reports FASN_PATH_VECTOR - also with a key-padding mask, with a bias next to
 * one, and with no mask or bias at all (FASN_PATH_PLAIN at head dims <= 128) - and FASN_PATH_ELEMENT otherwise. Without dropout, bias + key
 * padding at head dim 256 reports the family of the dense view of its mask (FASN_PATH_VECTOR or FASN_PATH_ELEMENT).
 */
#define FASN_PATH_PLAIN 0       /* no mask / bias (causal or not) */
#define FASN_PATH_KEYPAD 1      /* key-padding mask as per-tile visibility bits */
#define FASN_PATH_VECTOR 2      /* mask and / or bias through aligned vector loads / LDS images */
#define FASN_PATH_BIAS_KEYPAD 3 /* vector bias + key-padding visibility bits */
#define FASN_PATH_ELEMENT 4     /* per-element loads (slow) */
#define FASN_PATH_FP32 5        /* fp32 q/k/v: exact-fp32 MFMA kernels (1/16 of the 16-bit rate) */
int fasn_fwd_path(const fasn_fwd_args* args);

/*
 * Forward with a caller-provided workspace: short-query / long-key ("decode") shapes have too few (batch, head, query block)
 * units to fill the GPU, so the keys of each unit are split over several workgroups whose partial results
 * (fp32 accumulator + running max / sum per row) are merged by a second kernel. fasn_fwd_workspace_bytes() returns the
 * bytes that plan needs for `args` (0 = the plain path is used; fasn_fwd_ws then equals fasn_fwd). The workspace must be
 * 16-byte aligned device memory; a NULL or too small workspace silently selects the plain path. Same results either way.
 * Round 5, second use: LONG plain / causal launches at head dim 64 (8+ rounds of workgroups) ask for 64 bytes - eight item counters the
 * library zeroes itself - and then deal their (head, query block) items dynamically across the XCDs of the part (they differ in speed by up
 * to 4 %; a static deal ends with the slowest). Bit-identical results; without the workspace the static deal runs.
 */
size_t fasn_fwd_workspace_bytes(const fasn_fwd_args* args);
int fasn_fwd_ws(const fasn_fwd_args* args, void* workspace, size_t workspace_bytes, fasn_stream_t stream);

/*
 * Forward with a per-(batch, head) softmax_n (learned attention sinks: n_h = exp(s_h) is the weight of a per-head sink logit s_h, as
 * in GPT-OSS; the reference takes one n per call). Replaces fasn_fwd_ws when n is a tensor: `n` is a DEVICE pointer to fp32 values,
 * work item (b, h) reads n[b * n_stride_b + h * n_stride_h] (element strides >= 0, 0 = broadcast; h is the QUERY head, also under
 * kv_group) and args->softmax_n is ignored. The values are not checked (that would be a host round trip and break graph capture):
 * an entry that is not > 0 (0, negative, NaN) acts as n = 0. Same validation codes, workspace rule and kernel plan as fasn_fwd_ws
 * with the same args; a tensor filled with c gives bit for bit the results of softmax_n = c. n == NULL: exactly fasn_fwd_ws.
 * `n` must be 4-byte aligned (FASN_EALIGN) and (B-1) n_stride_b + (H-1) n_stride_h < 2^31 (FASN_EINVAL).
 */
int fasn_fwd_n(const fasn_fwd_args* args, const float* n, int64_t n_stride_b, int64_t n_stride_h, void* workspace,
               size_t workspace_bytes, fasn_stream_t stream);

/*
 * Gradient of that n (no counterpart in the reference, whose n carries none). With lse_i = log(n + sum_j exp(x_ij)) and
 * delta_i = sum_d dO_id O_id:
 *     dL/dn_(b,h) = - sum_i delta_i exp(-lse_i)        (rows with lse = -inf or lse < -2^22, and rows with delta_i = 0, add 0; unchanged under dropout: O is the dropped output)
 * Reads args->fwd.o, args->fwd.lse and args->dout (the views of the fasn_bwd call; nothing else of args is read beyond validation,
 * args->fwd.softmax_n is ignored), WRITES dn[b * dn_stride_b + h * dn_stride_h] as fp32. A stride of 0 asks for the sum over that
 * dimension (dn_stride_b = 0: sum over the batch, e.g. an n of shape [H]). Deterministic: a fixed-order two-stage reduction through
 * the caller's workspace (fasn_bwd_dn_workspace_bytes(args) bytes, 16-byte aligned; FASN_EWORKSPACE when missing or too small), no
 * atomics - the same inputs give the same bits. fasn_bwd needs no change for a tensor n: its kernels see n only through lse.
 * Two small kernels on `stream`; call it after (or before) fasn_bwd with the same args.
 */
size_t fasn_bwd_dn_workspace_bytes(const fasn_bwd_args* args);
int fasn_bwd_dn(const fasn_bwd_args* args, float* dn, int64_t dn_stride_b, int64_t dn_stride_h, void* workspace,
                size_t workspace_bytes, fasn_stream_t stream);

/*
 * Dropout stream position in device memory (replaces the host-side philox seed / offset bookkeeping behind
 * flash_attention_softmax_n/core/flash_attn.py:122 and functional.py:92): copies state[0..1] = {seed, offset} to out[0..1]
 * (out may be NULL) and advances state[1] by `increment`, as one tiny kernel on `stream` - capturable, no host round trip.
 * A forward call takes `out` as its rng_state; the backward of that call gets the same `out`.
 */
int fasn_rng_advance(uint64_t* state, uint64_t* out, uint64_t increment, fasn_stream_t stream);

size_t fasn_bwd_workspace_bytes(const fasn_bwd_args* args);
int fasn_bwd(const fasn_bwd_args* args, fasn_stream_t stream);

/*
 * The launches behind a call (ABI 5, the cfg field ABI 6; diagnostic like fasn_fwd_path, no counterpart in the reference, whose launch sites are
 * flash_attention_softmax_n/core/flash_attn_triton.py:278-291,316-335): runs the host side of fasn_fwd (FASN_PLAN_FWD, reads only
 * args->fwd), fasn_bwd (FASN_PLAN_BWD) or fasn_fwd_ws with the workspace it asks for (FASN_PLAN_FWD_WS) on `args` with every launch
 * site recording instead of launching, and writes one line per kernel into `buf`:
 *     "kernel_name<template arguments> grid=G block=T lds=L cfg=C\n"
 * (NUL-terminated; ABI 6: C names the template arguments of the kernel family - "bf16,D=64,QB=2,plain,OCC=2,NW=4,RING=2,SEED=2" for
 * fasn_fwd_kernel<fasn::bf16_tag, 64, 2, 0, 2, 4, 0, 0, 2, 0, 2, 1, 0, 0>: element type, head dim, 32-row blocks per wave, mode, waves per
 * SIMD the kernel is compiled for, waves per workgroup, K/V staging scheme, accumulator seeding; flags that are off are left out; "-" for a
 * kernel without a table - so that a plan, a profile line or a spill table reads without the kernel headers open). No kernel runs, no device memory is touched, no HIP call is made - pointers in `args` only have to be
 * non-NULL and aligned as for the real call. Returns the number of bytes written (without the NUL), the FASN_E* code the real
 * call would return, or FASN_EINVAL when `cap` is too small. The names are those of the code objects inside the library, so a
 * profile (rocprofv3 --kernel-trace) and a register / spill table (llvm-readelf on the bundle) can be matched against them.
 */
#define FASN_PLAN_FWD 0
#define FASN_PLAN_BWD 1
#define FASN_PLAN_FWD_WS 2
int fasn_launch_plan(const fasn_bwd_args* args, int32_t which, char* buf, size_t cap);

/*
 * Which kernel family the BACKWARD of a call takes (ABI 6): the value fasn_fwd_path gives for args->fwd, except that FASN_PATH_ELEMENT is
 * returned whenever the backward launches an element-load kernel. The question is put to the launch record itself (fasn_bwd under the
 * recorder of fasn_launch_plan, read as data: no plan text is written, so no length can make it fail), so that the front end's slow-path
 * warning follows the backward's launch table, not an assumption about it. Today the two only differ through operands the backward's kernels
 * cannot move as vectors although the forward's can (none known: since round 6 the head dim 256 backward has vector instantiations for dense
 * masks and 16-bit biases too). Argument rules and FASN_E* codes of fasn_bwd; nothing is launched.
 */
int fasn_bwd_path(const fasn_bwd_args* args);

/*
 * Forward over a K/V CACHE (inference; additions within ABI 6, no counterpart in the reference, which has no cache): attention of a few new
 * query positions per batch element (Sq = 1: decode) against keys that live in a paged or dense cache whose valid LENGTHS ARE IN DEVICE
 * MEMORY. Nothing about the lengths or the block table is read on the host: the launches depend on shapes and capacity only, so one
 * captured HIP graph serves every step of a generation while the sequences grow. Forward only; no mask other than the sliding window of the *_window calls below, no dropout, no bias other than the ALiBi slopes of the *_alibi calls.
 *
 *   cache     key j of batch element b is row j % page_size of page block_table[b * block_table_stride + j / page_size]; element
 *             (page, row, K/V head hk, feature d) of K sits at k_cache + (page * k_stride[0] + row * k_stride[1] + hk * k_stride[2] + d)
 *             elements (feature stride 1, every stride % 8, base 16-byte aligned). block_table == NULL is the dense cache: batch element b
 *             is one page of page_size (= its capacity) rows, page stride = batch stride; max_pages is ignored.
 *   lengths   len_b = clamp(seqlens[b] + seqlen_add, 0, capacity), capacity = max_pages * page_size (dense: page_size). Rows at or beyond
 *             len_b and pages beyond ceil(len_b / page_size) may hold anything (NaN bit patterns included) and never reach the result;
 *             block-table entries that are not needed are not read.
 *   rows      H % kv_group == 0; the kv_group query heads of a K/V head times the Sq positions are the rows of one problem (kv_group * Sq
 *             <= 128, else FASN_EUNSUPPORTED), so the cache is read once per K/V head; each row uses the softmax_n of its own query head:
 *             `n` / n_stride_b / n_stride_h with the meaning fasn_fwd_n gives them, n == NULL = the scalar softmax_n.
 *   causal    bottom-right aligned per batch element: position i sees key j iff j <= i + len_b - Sq. Rows that see no key give 0 and
 *             lse = log n (-inf for n = 0).
 *   supported D in {32, 64, 128, 256} - the head dims fasn_fwd has kernels for; every other size is FASN_EHEADDIM: a cache is never
 *             zero-padded - fp16 / bf16 (FASN_EDTYPE), paged: page_size % 64 == 0 at every head dim (FASN_EUNSUPPORTED). D = 256 runs
 *             one workgroup per CU (128 KiB of LDS) and its plans aim at ~512 workgroups where the other head dims aim at ~1024.
 *
 * fasn_fwd_kvcache needs fasn_fwd_kvcache_workspace_bytes(args) bytes of 16-byte aligned device memory (split partials; FASN_EWORKSPACE
 * when missing or too small) and launches two kernels. fasn_kvcache_append writes the Sq rows of k_new / v_new ([B, H / kv_group, Sq, D]
 * views) to the cache positions seqlens[b] .. seqlens[b] + Sq - 1 (seqlen_add is not used; positions at or beyond the capacity are dropped
 * inside the kernel; `seqlens` is not modified - the caller advances it); a forward that is to see them passes seqlen_add = Sq.
 * fasn_kvcache_plan writes the launches of fasn_fwd_kvcache as text, in the line format of fasn_launch_plan, without touching a device.
 */
typedef struct fasn_kvcache_args {
    fasn_view4 q;          /* [B,H,Sq,D] */
    fasn_view4 o;          /* [B,H,Sq,D] out */
    float* lse;            /* [B,H,Sq] fp32 contiguous, out; may be NULL */
    void* k_cache;
    void* v_cache;
    int64_t k_stride[3];   /* element strides (page, row, K/V head) */
    int64_t v_stride[3];
    const int32_t* block_table;  /* DEVICE [B, max_pages] page ids, or NULL (dense cache) */
    int64_t block_table_stride;  /* elements between the rows of two batch elements */
    int32_t max_pages;
    const int32_t* seqlens;      /* DEVICE [B] */
    int32_t seqlen_add;
    int32_t page_size;
    int32_t B, H, kv_group, Sq, D;
    int32_t dtype;         /* FASN_DTYPE_F16 / FASN_DTYPE_BF16 */
    float scale;
    float softmax_n;
    int32_t causal;
    const float* n;        /* DEVICE per-(batch, query head) softmax_n, or NULL */
    int64_t n_stride_b, n_stride_h;
} fasn_kvcache_args;

size_t fasn_fwd_kvcache_workspace_bytes(const fasn_kvcache_args* args);
int fasn_fwd_kvcache(const fasn_kvcache_args* args, void* workspace, size_t workspace_bytes, fasn_stream_t stream);
int fasn_kvcache_append(const fasn_kvcache_args* args, const fasn_view4* k_new, const fasn_view4* v_new, fasn_stream_t stream);
int fasn_kvcache_plan(const fasn_kvcache_args* args, char* buf, size_t cap);

/*
 * PREFILL over the same cache (additions within ABI 6): any number of query positions per batch element, Sq >= 1, with an optional
 * per-batch QUERY LENGTH IN DEVICE MEMORY. `kv` has the meaning fasn_fwd_kvcache gives it, and every rule and error code of that call
 * holds, except: there is no row limit (only kv_group > 128 is FASN_EUNSUPPORTED), and kv.seqlen_add is 0 (the cache as it is) or kv.Sq
 * (the cache plus the rows fasn_kvprefill_append wrote), anything else FASN_EINVAL.
 *
 *   lengths   qlen_b = clamp(q_seqlens[b], 0, Sq), q_seqlens == NULL = Sq: a ragged batch of prompts or chunks padded to Sq.
 *             len_b = clamp(seqlens[b] + (seqlen_add ? qlen_b : 0), 0, capacity).
 *   causal    position i < qlen_b sees key j iff j < len_b and (causal) j <= i + len_b - qlen_b: bottom-right aligned per batch element.
 *             A position that sees no key gives 0 and lse = log n (-inf for n = 0).
 *   padding   positions i >= qlen_b give o = 0 and lse = -inf whatever n is; their q / k_new / v_new rows are never read.
 *   rows      a workgroup owns the kv_group query heads of a K/V head times 128 / kv_group consecutive positions, so the cache is read
 *             once per K/V head and row block. The grid - (batch element, K/V head, row block, split) - depends on shapes and capacity only.
 *
 * fasn_fwd_kvprefill_workspace_bytes is 0 when the plan has one split (the forward kernel then stores o / lse itself, one launch; a NULL
 * workspace is accepted) and the size of the split partials otherwise (two launches; 16-byte aligned, FASN_EWORKSPACE when missing or too
 * small). fasn_kvprefill_append writes rows i < qlen_b of k_new / v_new ([B, H / kv_group, Sq, D] views) to the cache positions
 * seqlens[b] + i, drops positions at or beyond the capacity inside the kernel and does not modify `seqlens`. fasn_kvprefill_plan writes
 * the launches of fasn_fwd_kvprefill as text, in the line format of fasn_launch_plan, without touching a device.
 */
typedef struct fasn_kvprefill_args {
    fasn_kvcache_args kv;
    const int32_t* q_seqlens;    /* DEVICE [B] or NULL */
} fasn_kvprefill_args;

size_t fasn_fwd_kvprefill_workspace_bytes(const fasn_kvprefill_args* args);
int fasn_fwd_kvprefill(const fasn_kvprefill_args* args, void* workspace, size_t workspace_bytes, fasn_stream_t stream);
int fasn_kvprefill_append(const fasn_kvprefill_args* args, const fasn_view4* k_new, const fasn_view4* v_new, fasn_stream_t stream);
int fasn_kvprefill_plan(const fasn_kvprefill_args* args, char* buf, size_t cap);

/*
 * ALiBi SLOPES on the cache calls (additions within ABI 6; the argument blocks above keep their layouts): the logit of query position i
 * and key j becomes
 *     scale * q_i . k_j  -  slope[b, h] * | p_i - j |,      p_i = i + len_b - qlen_b      (decode: qlen_b = Sq)
 * with len_b / qlen_b as the base call defines them, read in device memory - p_i is the absolute position of query i, so a replayed graph
 * follows `seqlens` and `q_seqlens`. Visibility (causal, lengths, padding positions), the results of rows that see no key, softmax_n and
 * `n` are those of the base call; lse includes the bias. The bias is computed inside the forward kernels from the two integers and the
 * slope: no bias tensor exists. slope[b, h] = slopes[b * stride_b + h * stride_h] (fp32, DEVICE, h = query head; stride 0 broadcasts),
 * never read on the host.
 *
 * fasn_fwd_kvcache_alibi / fasn_fwd_kvprefill_alibi are fasn_fwd_kvcache / fasn_fwd_kvprefill with the operand: same launches, grids and
 * splits (kernels of their own for the forward, the same combine kernel), and the WORKSPACE of the base call -
 * fasn_fwd_kvcache_workspace_bytes(args) / fasn_fwd_kvprefill_workspace_bytes(args) bytes. The appends are the base calls'. Every rule
 * and error code of the base call holds and is checked first; then: alibi == NULL or slopes == NULL is FASN_EINVAL, slopes not 4-byte
 * aligned FASN_EALIGN, a negative stride or (B-1) stride_b + (H-1) stride_h >= 2^31 FASN_EINVAL. The *_alibi_plan calls are
 * fasn_kvcache_plan / fasn_kvprefill_plan for these launches.
 */
typedef struct fasn_alibi_slopes {
    const float* slopes;         /* DEVICE per-(batch, query head) slope */
    int64_t stride_b, stride_h;  /* elements */
} fasn_alibi_slopes;

int fasn_fwd_kvcache_alibi(const fasn_kvcache_args* args, const fasn_alibi_slopes* alibi, void* workspace, size_t workspace_bytes, fasn_stream_t stream);
int fasn_fwd_kvprefill_alibi(const fasn_kvprefill_args* args, const fasn_alibi_slopes* alibi, void* workspace, size_t workspace_bytes, fasn_stream_t stream);
int fasn_kvcache_alibi_plan(const fasn_kvcache_args* args, const fasn_alibi_slopes* alibi, char* buf, size_t cap);
int fasn_kvprefill_alibi_plan(const fasn_kvprefill_args* args, const fasn_alibi_slopes* alibi, char* buf, size_t cap);

/*
 * SLIDING WINDOW on the cache calls (additions within ABI 6; the argument blocks above keep their layouts): always causal, position
 *     p_i = i + len_b - qlen_b      (decode: qlen_b = Sq; len_b / qlen_b as the base call defines them, clamps and append included)
 * sees key j iff j < len_b and p_i - window < j <= p_i: `window` keys, the position's own included (Hugging Face sliding_window,
 * GPT-OSS, Mistral). `window` is a host integer >= 1 - a per-layer constant, part of a captured graph - while the lengths stay in device
 * memory. softmax_n, `n`, scale and lse are the base call's: lse covers the visible keys plus n, a position that sees no key (p_i < 0)
 * gives 0 and lse = log n, padding positions give 0 and -inf.
 *
 * MEMORY CONTRACT. With first_b = 64 * floor(max(0, len_b - qlen_b - window + 1) / 64):
 *   - cache rows j < first_b are never read, and neither are the block-table entries of pages that lie wholly below first_b: both may
 *     hold anything (NaN, a freed page, a page that serves somebody else) - a server may free every page wholly below the window;
 *   - rows first_b .. len_b - 1 are read in tiles of 64 keys and must hold finite values (they are rows an earlier append wrote);
 *   - rows at or beyond len_b keep the base call's rule: out of range for the tile's descriptor, they arrive as zeros.
 *
 * fasn_fwd_kvcache_window / fasn_fwd_kvprefill_window are fasn_fwd_kvcache / fasn_fwd_kvprefill with the operand: forward kernels of
 * their own, the same combine kernels, the appends of the base calls. The plan uses the window - a workgroup walks at most
 * ceil((window + span - 1) / 64) + 1 tiles (span = Sq, prefill: 128 / kv_group), which takes the place of the capacity's tiles in the
 * split rule - so the workspace is fasn_fwd_kv{cache,prefill}_window_workspace_bytes(args, window), never more than the base call's
 * (prefill: 0 with one split). A window >= capacity gives the base plan under the window kernels' names. Every rule and error code of the
 * base call holds and is checked first; then window == NULL, window->window < 1 or reserved != 0 is FASN_EINVAL and args->causal == 0
 * FASN_EUNSUPPORTED; any window >= 1 is legal (one beyond the capacity acts as the capacity). There is no window + ALiBi call. The
 * *_window_plan calls are fasn_kvcache_plan / fasn_kvprefill_plan for these launches.
 */
typedef struct fasn_kv_window {
    int32_t window;              /* keys a position sees, its own included; >= 1 */
    int32_t reserved;            /* 0 */
} fasn_kv_window;

size_t fasn_fwd_kvcache_window_workspace_bytes(const fasn_kvcache_args* args, const fasn_kv_window* window);
int fasn_fwd_kvcache_window(const fasn_kvcache_args* args, const fasn_kv_window* window, void* workspace, size_t workspace_bytes, fasn_stream_t stream);
int fasn_kvcache_window_plan(const fasn_kvcache_args* args, const fasn_kv_window* window, char* buf, size_t cap);
size_t fasn_fwd_kvprefill_window_workspace_bytes(const fasn_kvprefill_args* args, const fasn_kv_window* window);
int fasn_fwd_kvprefill_window(const fasn_kvprefill_args* args, const fasn_kv_window* window, void* workspace, size_t workspace_bytes, fasn_stream_t stream);
int fasn_kvprefill_window_plan(const fasn_kvprefill_args* args, const fasn_kv_window* window, char* buf, size_t cap);

/*
 * ROTARY POSITION EMBEDDING on the cache calls (additions within ABI 6; the argument blocks above keep their layouts): one launch that
 * takes the place of the append in front of a forward. With len_b / qlen_b as the base call defines them (clamps included, read in
 * device memory - a replayed graph follows `seqlens` and `q_seqlens`):
 *   k_new   row i < qlen_b of k_new[b, hk] is rotated at position seqlens[b] + i and written to that cache row, addressed as
 *           fasn_kvcache_append addresses it; rows at a negative position or at / beyond the capacity are dropped inside the kernel
 *   v_new   row i < qlen_b is copied to the same position, unrotated
 *   q       row i < qlen_b of args->q[b, h] is rotated at p_i = i + len_b - qlen_b (decode: qlen_b = Sq) - the p_i of the *_alibi and
 *           *_window calls - and written to q_out[b, h, i]; rows i >= qlen_b are neither read nor written (the forward never reads them)
 * k_new == v_new == NULL: only the queries are rotated, with args->seqlen_add as given. With k_new / v_new, seqlen_add must be Sq.
 *
 *   layouts   features d < rotary_dim are rotated, the others copied. With c = cos[pos, d], s = sin[pos, d], d < rotary_dim / 2:
 *             interleaved = 0 (GPT-NeoX / Llama / GPT-OSS, Hugging Face rotate_half): x1 = x[d], x2 = x[d + rotary_dim / 2];
 *             interleaved = 1 (GPT-J): x1 = x[2 d], x2 = x[2 d + 1];   y1 = x1 c - x2 s, y2 = x2 c + x1 s, written where x1 / x2 were.
 *   tables    cos / sin [rows, rotary_dim / 2], fp32 (FASN_DTYPE_F32, defined below) or the dtype of `args`, DEVICE, column stride 1.
 *             The row read is clamp(pos, 0, rows - 1); rows >= capacity, so the clamp acts only on the negative p_i of causal rows that
 *             see no key. Scaling rules (YaRN, NTK, an attention factor) live in the tables.
 *   rounding  operands widened to fp32; each product rounded to fp32 on its own, the sum / difference rounded to fp32 on its own (no
 *             fused multiply-add), one rounding to the 16-bit type, to nearest even: bit for bit (x1 c - x2 s) evaluated in fp32 step by step.
 *
 * CALL SEQUENCE of one layer step: fasn_kvcache_rope_append(args, rope, &q_out, &k_new, &v_new, stream) with args->seqlen_add = Sq, then
 * fasn_fwd_kvcache (or fasn_fwd_kvcache_window) on the same args with args->q = q_out; the prefill calls alike. It replaces
 * fasn_kvcache_append / fasn_kvprefill_append: launches per step do not change. `seqlens` is not modified.
 *
 * Every rule and error code of the base call holds and is checked first; then: rope, cos, sin or q_out NULL, k_new and v_new not both
 * NULL or both given, k_new given with seqlen_add != Sq, rotary_dim outside [16, D] or not a multiple of 16, rows < capacity, interleaved
 * not 0 or 1, row_stride < rotary_dim / 2 are FASN_EINVAL; table_dtype neither FASN_DTYPE_F32 nor args->dtype is FASN_EDTYPE; a table
 * base that is not 16-byte aligned or a row stride that is not a multiple of 16 bytes is FASN_EALIGN; q_out, k_new, v_new follow the
 * rules of q with its codes. The *_plan calls write the one launch as text, in the line format of fasn_launch_plan, without touching a
 * device: its grid is ceil(((k_new ? B * (H / kv_group) * Sq : 0) + B * H * Sq) * (D / 16) / 256) workgroups - shapes only.
 */
typedef struct fasn_kv_rope {
    const void* cos;             /* DEVICE [rows, rotary_dim / 2], unit column stride */
    const void* sin;
    int64_t row_stride;          /* elements */
    int32_t rows;                /* positions the tables cover; >= capacity */
    int32_t rotary_dim;          /* 16 <= rotary_dim <= D, % 16 == 0 */
    int32_t table_dtype;         /* FASN_DTYPE_F32, or the dtype of args */
    int32_t interleaved;         /* 0 half-split, 1 (2d, 2d+1) pairs */
} fasn_kv_rope;

int fasn_kvcache_rope_append(const fasn_kvcache_args* args, const fasn_kv_rope* rope, const fasn_view4* q_out, const fasn_view4* k_new,
                             const fasn_view4* v_new, fasn_stream_t stream);
int fasn_kvprefill_rope_append(const fasn_kvprefill_args* args, const fasn_kv_rope* rope, const fasn_view4* q_out, const fasn_view4* k_new,
                               const fasn_view4* v_new, fasn_stream_t stream);
int fasn_kvcache_rope_append_plan(const fasn_kvcache_args* args, const fasn_kv_rope* rope, const fasn_view4* q_out, const fasn_view4* k_new,
                                  const fasn_view4* v_new, char* buf, size_t cap);
int fasn_kvprefill_rope_append_plan(const fasn_kvprefill_args* args, const fasn_kv_rope* rope, const fasn_view4* q_out,
                                    const fasn_view4* k_new, const fasn_view4* v_new, char* buf, size_t cap);

/*
 * PREFILL ON TOKEN-PACKED QUERIES (continuous batching; additions within ABI 6, the argument blocks above keep their layouts): the query
 * positions of all sequences of a step lie behind each other in one buffer of total_tokens rows, and cu_seqlens_q - B + 1 int32 offsets in
 * DEVICE memory, cu[0] = 0, non-decreasing, cu[B] <= total_tokens - says where each sequence starts (vLLM's flash_attn_varlen_func with a
 * block table). A step of many one-token sequences and a few long chunks costs what its tokens cost, not B times the longest chunk.
 *
 *   pf.kv     as fasn_fwd_kvprefill takes it, with: B = the number of sequences; Sq = max_seqlen_q >= 1, a host bound of every query
 *             length (a constant of a captured graph); q / o = views of [1, H, total_tokens, D]: stride[1] between heads, stride[2]
 *             between tokens, stride[0] unused; lse = [H, total_tokens] fp32 or NULL; seqlen_add = 0 or Sq as in the prefill call.
 *             pf.q_seqlens must be NULL (FASN_EINVAL): the lengths come from the offsets.
 *   lengths   qlen_b = clamp(cu[b + 1] - cu[b], 0, Sq); token cu[b] + i is position i < qlen_b of sequence b; len_b, visibility, the
 *             result of a position that sees no key, `n` ([B, H]: per sequence, not per token) and scale are the prefill call's.
 *   tokens    at or beyond cu[B] are never read; their o / lse rows are not written.
 *   safety    nothing is read on the host. Whatever cu_seqlens_q holds, no kernel touches memory outside the buffers: token indices are
 *             clamped to [0, total_tokens), lengths as above. Malformed offsets give unspecified values in o / lse / the appended rows.
 *
 * fasn_fwd_kvvarlen launches a schedule kernel - offsets -> a table of (sequence, row block) items in the workspace - the forward on
 * items_max * (H / kv_group) * nsplit workgroups, items_max = min(B * ceil(Sq / PB), total_tokens / PB + B), PB = 128 / kv_group, and with
 * several splits a combine kernel. One split count serves the whole launch, from shapes and capacity: the prefill rule over
 * items_max * (H / kv_group) blocks. The workspace (fasn_fwd_kvvarlen_workspace_bytes, never 0: the table, then the split partials) is
 * always needed: 16-byte aligned, FASN_EWORKSPACE when missing or too small. fasn_kvvarlen_append writes token t of k_new / v_new (views
 * of [1, H / kv_group, total_tokens, D]) to cache row seqlens[b] + t - cu[b] of its sequence under the rules of fasn_kvprefill_append.
 * fasn_kvvarlen_plan writes the launches of fasn_fwd_kvvarlen as text. Every rule and error code of fasn_fwd_kvprefill holds and is checked
 * first; then cu_seqlens_q == NULL, pf.q_seqlens != NULL, total_tokens < 1 or reserved != 0 is FASN_EINVAL, offsets that are not 4-byte
 * aligned FASN_EALIGN, a table beyond 2^31 / 128 / (H / kv_group) items FASN_EINVAL.
 *
 * SLIDING WINDOW AND ROTARY EMBEDDING ON PACKED QUERIES (additions within ABI 6): the packed siblings of the *_window and *_rope_append
 * calls above, with their operands, their semantics per sequence (p_i = i + len_b - qlen_b, the memory contract of the window with
 * first_b = 64 * floor(max(0, len_b - qlen_b - window + 1) / 64), the layouts, tables and rounding of the rotation) and their codes.
 *   fasn_fwd_kvvarlen_window     fasn_fwd_kvvarlen with a forward kernel of its own; the schedule and combine kernels are the same. The
 *                                split rule runs over items_max * (H / kv_group) blocks and the tiles a window can touch, so the workspace
 *                                is fasn_fwd_kvvarlen_window_workspace_bytes(args, window): the table, then the partials, never more than
 *                                the base call's. fasn_kvvarlen_window_plan writes its launches.
 *   fasn_kvvarlen_rope_append    ONE launch in the place of fasn_kvvarlen_append: token cu[b] + i of k_new is rotated at position
 *                                seqlens[b] + i into the cache (dropped at a negative position or at / beyond the capacity), v_new copied
 *                                beside it, the query token rotated at p_i into q_out; q_out, k_new, v_new are views of
 *                                [1, heads, total_tokens, D]. Tokens at or beyond cu[B] are neither read nor written. The forward that
 *                                follows reads q_out in the place of q. Its grid is
 *                                ceil(((k_new ? total_tokens * (H / kv_group) : 0) + total_tokens * H) * (D / 16) / 256): shapes only.
 * Every rule and error code of fasn_fwd_kvvarlen holds and is checked first, then the operand's rules with the operand's codes, before
 * any HIP call. There is no packed ALiBi call.
 */
typedef struct fasn_kvvarlen_args {
    fasn_kvprefill_args pf;
    const int32_t* cu_seqlens_q; /* DEVICE [B + 1] token offsets */
    int32_t total_tokens;        /* rows of the token buffers; >= 1 */
    int32_t reserved;            /* 0 */
} fasn_kvvarlen_args;

size_t fasn_fwd_kvvarlen_workspace_bytes(const fasn_kvvarlen_args* args);
int fasn_fwd_kvvarlen(const fasn_kvvarlen_args* args, void* workspace, size_t workspace_bytes, fasn_stream_t stream);
int fasn_kvvarlen_append(const fasn_kvvarlen_args* args, const fasn_view4* k_new, const fasn_view4* v_new, fasn_stream_t stream);
int fasn_kvvarlen_plan(const fasn_kvvarlen_args* args, char* buf, size_t cap);
size_t fasn_fwd_kvvarlen_window_workspace_bytes(const fasn_kvvarlen_args* args, const fasn_kv_window* window);
int fasn_fwd_kvvarlen_window(const fasn_kvvarlen_args* args, const fasn_kv_window* window, void* workspace, size_t workspace_bytes, fasn_stream_t stream);
int fasn_kvvarlen_window_plan(const fasn_kvvarlen_args* args, const fasn_kv_window* window, char* buf, size_t cap);
int fasn_kvvarlen_rope_append(const fasn_kvvarlen_args* args, const fasn_kv_rope* rope, const fasn_view4* q_out, const fasn_view4* k_new,
                              const fasn_view4* v_new, fasn_stream_t stream);
int fasn_kvvarlen_rope_append_plan(const fasn_kvvarlen_args* args, const fasn_kv_rope* rope, const fasn_view4* q_out, const fasn_view4* k_new,
                                   const fasn_view4* v_new, char* buf, size_t cap);

/*
 * TOKEN-TREE ATTENTION on the cache calls (speculative-decoding verification: EAGLE, Medusa, SpecInfer; additions within ABI 6, the
 * argument blocks above keep their layouts). The qlen_b new positions of a batch element are the NODES of a tree of draft tokens, in the
 * order of q. With len_b / qlen_b as the base call defines them (clamps and append included) and base_b = len_b - qlen_b:
 *   rows       node i sits in cache row base_b + i.
 *   mask       int64 words in DEVICE memory, word (b, i) at mask[b * batch_stride + i], i < Sq <= 64. Bit t says that node i sees node t;
 *              bits t >= qlen_b are ignored, bit 63 (the sign bit) is an ordinary bit.
 *   sees       node i sees key j iff j < base_b (the prefix; under a window also j > p_i - window), or j = base_b + t with t < qlen_b
 *              and bit t set.
 *   position   p_i = base_b + d_i, d_i = max(popcount(word & the low qlen_b bits) - 1, 0): a well-formed row holds the node itself and
 *              exactly its ancestors, so popcount - 1 is its depth and no position tensor exists.
 *   anything   may stand in the mask - upper-triangular bits, a missing self bit, an all-zero row: the result is what the rule says and
 *              no access depends on the mask. A row that sees nothing gives 0 and lse = log n (-inf for n = 0); positions i >= qlen_b
 *              give 0 / -inf and are neither read nor rotated.
 *   window     0: none; >= 1: first_b = 64 * floor(max(0, base_b - window + 1) / 64), and pages wholly below first_b are never read -
 *              neither their rows nor their table entries (the MEMORY CONTRACT of the *_window calls).
 * softmax_n, `n`, scale, lse, split-K, the combine kernels and the stale-memory rules are the base call's.
 *
 *   fasn_fwd_kvcache_tree / fasn_fwd_kvprefill_tree   the base call with the operand: one forward kernel of their own each (the window is a
 *              run-time integer of it), the same combine kernels, the appends of the base calls. The plan is the base call's rule; with a
 *              window it is the *_window rule with span Sq (every row block walks the window of all Sq nodes). The workspace is
 *              fasn_fwd_kv{cache,prefill}_tree_workspace_bytes(args, tree); the *_tree_plan calls write the launches as text.
 *   fasn_kvcache_tree_rope_append / fasn_kvprefill_tree_rope_append   the *_rope_append call at DEPTH positions: node i of k_new is
 *              written to cache row seqlens[b] + i but rotated at seqlens[b] + d_i, the query node at p_i. Everything else is the
 *              *_rope_append call's (tree->window takes no part).
 *   fasn_kvcache_tree_commit   after acceptance: for k < clamp(accepted_lens[b], 0, A) the K and V rows seqlens[b] + accepted[b, k] move
 *              to the rows seqlens[b] + k, through the block table; seqlens[b] = base_b, the prefix length that was passed to the tree
 *              call. A path is strictly increasing (accepted[b, k] >= k); an index outside [k, nodes) or a row at / beyond the capacity
 *              skips that move, so a malformed path gives unspecified rows and never touches memory outside the cache. accepted[b, k] == k
 *              moves nothing. `seqlens` is not modified. Rotated keys need no re-rotation: node k of a path has depth k and lands at the
 *              position it was rotated for.
 * Every rule and error code of the base call holds and is checked first (the rope calls: then the rope operand's); then tree == NULL,
 * mask == NULL or reserved != 0 is FASN_EINVAL, Sq > 64 FASN_EUNSUPPORTED, args->causal == 0 FASN_EUNSUPPORTED, window < 0 FASN_EINVAL,
 * a mask that is not 8-byte aligned FASN_EALIGN and a negative batch_stride FASN_EINVAL. Not here: ALiBi, packed queries, gradients.
 */
typedef struct fasn_kv_tree {
    const int64_t* mask;         /* DEVICE, word (b, i) at mask[b * batch_stride + i] */
    int64_t batch_stride;        /* elements */
    int32_t window;              /* 0: none; >= 1: the sliding window of the *_window calls */
    int32_t reserved;            /* 0 */
} fasn_kv_tree;

typedef struct fasn_kv_tree_commit {
    void* k_cache;               /* the cache as fasn_kvcache_args names it: pools, strides, table, lengths, page size */
    void* v_cache;
    int64_t k_stride[3];
    int64_t v_stride[3];
    const int32_t* block_table;
    int64_t block_table_stride;
    int32_t max_pages;
    int32_t page_size;
    const int32_t* seqlens;      /* DEVICE [B]: base_b, the prefix length */
    int32_t B;
    int32_t Hkv;                 /* K/V heads */
    int32_t D;                   /* 32, 64, 128, 256; 16-bit elements (fasn_kvcache_fp8_tree_commit: 64, 128; codes) */
    int32_t A;                   /* columns of accepted, 1 .. 64 */
    const int32_t* accepted;     /* DEVICE, node (b, k) at accepted[b * accepted_stride + k] */
    int64_t accepted_stride;     /* elements, >= A */
    const int32_t* accepted_lens;/* DEVICE [B] */
    int32_t nodes;               /* node indices lie in [0, nodes), 1 .. 64: the Sq of the tree call */
    int32_t reserved;            /* 0 */
} fasn_kv_tree_commit;

size_t fasn_fwd_kvcache_tree_workspace_bytes(const fasn_kvcache_args* args, const fasn_kv_tree* tree);
int fasn_fwd_kvcache_tree(const fasn_kvcache_args* args, const fasn_kv_tree* tree, void* workspace, size_t workspace_bytes, fasn_stream_t stream);
int fasn_kvcache_tree_plan(const fasn_kvcache_args* args, const fasn_kv_tree* tree, char* buf, size_t cap);
size_t fasn_fwd_kvprefill_tree_workspace_bytes(const fasn_kvprefill_args* args, const fasn_kv_tree* tree);
int fasn_fwd_kvprefill_tree(const fasn_kvprefill_args* args, const fasn_kv_tree* tree, void* workspace, size_t workspace_bytes, fasn_stream_t stream);
int fasn_kvprefill_tree_plan(const fasn_kvprefill_args* args, const fasn_kv_tree* tree, char* buf, size_t cap);
int fasn_kvcache_tree_rope_append(const fasn_kvcache_args* args, const fasn_kv_rope* rope, const fasn_kv_tree* tree, const fasn_view4* q_out,
                                  const fasn_view4* k_new, const fasn_view4* v_new, fasn_stream_t stream);
int fasn_kvprefill_tree_rope_append(const fasn_kvprefill_args* args, const fasn_kv_rope* rope, const fasn_kv_tree* tree, const fasn_view4* q_out,
                                    const fasn_view4* k_new, const fasn_view4* v_new, fasn_stream_t stream);
int fasn_kvcache_tree_commit(const fasn_kv_tree_commit* commit, fasn_stream_t stream);

/*
 * FP8 K/V CACHE (additions within ABI 6): the base decode and prefill calls over a cache of OCP e4m3fn codes (torch.float8_e4m3fn;
 * gfx950's FP8, not MI300's fnuz) with one fp32 scale per (batch element, K/V head) in device memory. One operand beside the unchanged
 * argument blocks. In those blocks k_cache / v_cache point at BYTES, k_stride / v_stride count elements (= bytes) and `dtype` is the
 * dtype of q, o, k_new and v_new (fp16 / bf16).
 *
 *   value      of a cache element = up(code) * scale[b, hkv], up() the exact upcast: all 254 finite codes are fp16 and bf16 numbers, so
 *              the 16-bit MFMAs take the codes themselves and the scales act in fp32 only:
 *                x_ij  = scale * k_scale[b, hkv] * (q_i . up(Kc_j))
 *                out_i = v_scale[b, hkv] * sum_j p_ij up(Vc_j) / (n + sum_j p_ij)        rounded once, after the scale
 *              No Q or P quantisation, no fp8 MFMA. A NaN code in a visible row is a NaN, as a NaN in a 16-bit cache is.
 *   scales     scale (b, hkv) at k_scale[b * k_sb + hkv * k_sh] (v likewise): the rules of `n`, per K/V head; stride 0 broadcasts. Read
 *              by the kernels only - a captured graph follows them. A non-positive or non-finite scale gives unspecified results and
 *              touches no memory outside the buffers.
 *   append     fasn_kv{cache,prefill}_fp8_append: code = rne_e4m3(clamp(float(x) / s, -448, 448)), s the scale of the row's (b, hkv), the
 *              division correctly rounded in fp32, NaN -> a NaN code; rows, positions and the dropping beyond the capacity as
 *              fasn_kv{cache,prefill}_append.
 *   the rest   visibility, len_b / qlen_b, seqlen_add, softmax_n and `n`, the sink on split 0, lse, rows that see nothing, the
 *              stale-memory rules (rows at or beyond len_b may hold any byte, 0x7f included), the split rule and the workspace size are
 *              the base call's: fasn_fwd_kv{cache,prefill}_fp8_workspace_bytes, the *_fp8_plan calls write the launches as text.
 * Every rule and error code of the base call holds and is checked first; then fp8 == NULL, a NULL scale or reserved != 0 is FASN_EINVAL,
 * D other than 64 / 128 FASN_EHEADDIM, a scale pointer off 4 bytes or a cache stride that is not a multiple of 16 (bytes) FASN_EALIGN, a
 * negative or overflowing scale stride FASN_EINVAL. Not here: ALiBi, e5m2, gradients; windows, rotary appends and trees have calls of
 * their own below, packed queries the operand-set calls at the end of the cache section.
 */
typedef struct fasn_kv_fp8 {
    const float* k_scale;        /* DEVICE */
    const float* v_scale;        /* DEVICE */
    int64_t k_sb;                /* element strides (batch, K/V head) */
    int64_t k_sh;
    int64_t v_sb;
    int64_t v_sh;
    int32_t reserved;            /* 0 */
} fasn_kv_fp8;

size_t fasn_fwd_kvcache_fp8_workspace_bytes(const fasn_kvcache_args* args, const fasn_kv_fp8* fp8);
int fasn_fwd_kvcache_fp8(const fasn_kvcache_args* args, const fasn_kv_fp8* fp8, void* workspace, size_t workspace_bytes, fasn_stream_t stream);
int fasn_kvcache_fp8_plan(const fasn_kvcache_args* args, const fasn_kv_fp8* fp8, char* buf, size_t cap);
int fasn_kvcache_fp8_append(const fasn_kvcache_args* args, const fasn_kv_fp8* fp8, const fasn_view4* k_new, const fasn_view4* v_new,
                            fasn_stream_t stream);
size_t fasn_fwd_kvprefill_fp8_workspace_bytes(const fasn_kvprefill_args* args, const fasn_kv_fp8* fp8);
int fasn_fwd_kvprefill_fp8(const fasn_kvprefill_args* args, const fasn_kv_fp8* fp8, void* workspace, size_t workspace_bytes, fasn_stream_t stream);
int fasn_kvprefill_fp8_plan(const fasn_kvprefill_args* args, const fasn_kv_fp8* fp8, char* buf, size_t cap);
int fasn_kvprefill_fp8_append(const fasn_kvprefill_args* args, const fasn_kv_fp8* fp8, const fasn_view4* k_new, const fasn_view4* v_new,
                              fasn_stream_t stream);

/*
 * FP8 K/V CACHE, THE LAYER (additions within ABI 6; no struct is new or changed): the sliding window and the rotary append over the FP8
 * cache above - what a GPT-OSS / Mistral / Llama layer needs of it. Decode and prefill blocks only; a packed block has no such NAMED call
 * (fasn_kv_forward / fasn_kv_append below take it).
 *
 *   window     fasn_fwd_kv{cache,prefill}_fp8_window: fasn_fwd_kv{cache,prefill}_window's visibility, tile walk and memory contract (rows
 *              and block-table entries below the window's first tile are never read) with the FP8 call's values and scales. The plan
 *              is the 16-bit window call's of the same shape and window - same grids, same workspace - with the FP8 kernels' LDS.
 *              Checks: the base call's, then the FP8 operand's (as fasn_fwd_kv*_fp8), then the window's (window == NULL, window < 1 or
 *              reserved != 0: FASN_EINVAL; a non-causal block: FASN_EUNSUPPORTED).
 *   rope       fasn_kv{cache,prefill}_fp8_rope_append: fasn_kv{cache,prefill}_rope_append in front of an FP8 cache, ONE launch on the
 *              same grid. q_out is that call's (16-bit). A key row is rotated and rounded once to `dtype` exactly as that call stores
 *              it, and THAT value is quantised as fasn_kv*_fp8_append quantises k_new - code = rne_e4m3(clamp(float(x) / k_scale,
 *              -448, 448)), NaN -> a NaN code - so the call equals "rotate in eager fp32 arithmetic, round to dtype, fasn_kv*_fp8_append"
 *              byte for byte. Features at or beyond rotary_dim are quantised unrotated; v_new is quantised with v_scale. Positions,
 *              dropped rows, padding rows and the table-row clamp are the 16-bit call's. k_new == v_new == NULL: queries only.
 *              Checks: the base call's, then the FP8 operand's, then the rope operand's (as fasn_kv*_rope_append). The tree variant
 *              is fasn_kv{cache,prefill}_fp8_tree_rope_append below.
 */
size_t fasn_fwd_kvcache_fp8_window_workspace_bytes(const fasn_kvcache_args* args, const fasn_kv_fp8* fp8, const fasn_kv_window* window);
int fasn_fwd_kvcache_fp8_window(const fasn_kvcache_args* args, const fasn_kv_fp8* fp8, const fasn_kv_window* window, void* workspace,
                                size_t workspace_bytes, fasn_stream_t stream);
int fasn_kvcache_fp8_window_plan(const fasn_kvcache_args* args, const fasn_kv_fp8* fp8, const fasn_kv_window* window, char* buf, size_t cap);
size_t fasn_fwd_kvprefill_fp8_window_workspace_bytes(const fasn_kvprefill_args* args, const fasn_kv_fp8* fp8, const fasn_kv_window* window);
int fasn_fwd_kvprefill_fp8_window(const fasn_kvprefill_args* args, const fasn_kv_fp8* fp8, const fasn_kv_window* window, void* workspace,
                                  size_t workspace_bytes, fasn_stream_t stream);
int fasn_kvprefill_fp8_window_plan(const fasn_kvprefill_args* args, const fasn_kv_fp8* fp8, const fasn_kv_window* window, char* buf, size_t cap);
int fasn_kvcache_fp8_rope_append(const fasn_kvcache_args* args, const fasn_kv_fp8* fp8, const fasn_kv_rope* rope, const fasn_view4* q_out,
                                 const fasn_view4* k_new, const fasn_view4* v_new, fasn_stream_t stream);
int fasn_kvprefill_fp8_rope_append(const fasn_kvprefill_args* args, const fasn_kv_fp8* fp8, const fasn_kv_rope* rope, const fasn_view4* q_out,
                                   const fasn_view4* k_new, const fasn_view4* v_new, fasn_stream_t stream);
int fasn_kvcache_fp8_rope_append_plan(const fasn_kvcache_args* args, const fasn_kv_fp8* fp8, const fasn_kv_rope* rope, const fasn_view4* q_out,
                                      const fasn_view4* k_new, const fasn_view4* v_new, char* buf, size_t cap);
int fasn_kvprefill_fp8_rope_append_plan(const fasn_kvprefill_args* args, const fasn_kv_fp8* fp8, const fasn_kv_rope* rope, const fasn_view4* q_out,
                                        const fasn_view4* k_new, const fasn_view4* v_new, char* buf, size_t cap);

/*
 * FP8 K/V CACHE, TOKEN TREES (additions within ABI 6; no struct is new or changed): the token-tree calls above over the FP8 cache -
 * speculative-decoding verification without dequantising the cache. Decode and prefill blocks only.
 *
 *   forward    fasn_fwd_kv{cache,prefill}_fp8_tree: fasn_fwd_kv{cache,prefill}_tree's rows, mask, visibility, positions, window and memory
 *              contract with the FP8 call's values and scales. The plan is the 16-bit tree call's of the same shape and window - same
 *              grids, same split counts, same workspace - with the FP8 kernels' LDS and combine kernels. The append without rotary is
 *              fasn_kv{cache,prefill}_fp8_append.
 *   rope       fasn_kv{cache,prefill}_fp8_tree_rope_append: fasn_kv{cache,prefill}_fp8_rope_append at DEPTH positions, ONE launch on the
 *              grid of fasn_kv{cache,prefill}_tree_rope_append. Node i of k_new is written to cache row seqlens[b] + i but rotated at
 *              seqlens[b] + d_i, rounded once to `dtype` and quantised with k_scale; v_new is quantised beside it; the query node is
 *              rotated at p_i. tree->window takes no part. The *_fp8_tree_rope_append_plan calls write the launch as text.
 *   commit     fasn_kvcache_fp8_tree_commit: fasn_kvcache_tree_commit over code rows, with the same fasn_kv_tree_commit block. D is 64
 *              or 128 (anything else: FASN_EHEADDIM), k_stride / v_stride count codes and are multiples of 16 (FASN_EALIGN), the pools
 *              are 16-byte aligned, reserved is 0; every other rule and code is that call's.
 * Checks, in this order: the base call's, the FP8 operand's (as fasn_fwd_kv*_fp8), the tree operand's (as fasn_fwd_kv*_tree, the same
 * codes), and on the rope calls the rope operand's. Not here: packed trees, ALiBi, D = 32 / 256, e5m2, gradients.
 */
size_t fasn_fwd_kvcache_fp8_tree_workspace_bytes(const fasn_kvcache_args* args, const fasn_kv_fp8* fp8, const fasn_kv_tree* tree);
int fasn_fwd_kvcache_fp8_tree(const fasn_kvcache_args* args, const fasn_kv_fp8* fp8, const fasn_kv_tree* tree, void* workspace,
                              size_t workspace_bytes, fasn_stream_t stream);
int fasn_kvcache_fp8_tree_plan(const fasn_kvcache_args* args, const fasn_kv_fp8* fp8, const fasn_kv_tree* tree, char* buf, size_t cap);
size_t fasn_fwd_kvprefill_fp8_tree_workspace_bytes(const fasn_kvprefill_args* args, const fasn_kv_fp8* fp8, const fasn_kv_tree* tree);
int fasn_fwd_kvprefill_fp8_tree(const fasn_kvprefill_args* args, const fasn_kv_fp8* fp8, const fasn_kv_tree* tree, void* workspace,
                                size_t workspace_bytes, fasn_stream_t stream);
int fasn_kvprefill_fp8_tree_plan(const fasn_kvprefill_args* args, const fasn_kv_fp8* fp8, const fasn_kv_tree* tree, char* buf, size_t cap);
int fasn_kvcache_fp8_tree_rope_append(const fasn_kvcache_args* args, const fasn_kv_fp8* fp8, const fasn_kv_rope* rope, const fasn_kv_tree* tree,
                                      const fasn_view4* q_out, const fasn_view4* k_new, const fasn_view4* v_new, fasn_stream_t stream);
int fasn_kvprefill_fp8_tree_rope_append(const fasn_kvprefill_args* args, const fasn_kv_fp8* fp8, const fasn_kv_rope* rope, const fasn_kv_tree* tree,
                                        const fasn_view4* q_out, const fasn_view4* k_new, const fasn_view4* v_new, fasn_stream_t stream);
int fasn_kvcache_fp8_tree_rope_append_plan(const fasn_kvcache_args* args, const fasn_kv_fp8* fp8, const fasn_kv_rope* rope, const fasn_kv_tree* tree,
                                           const fasn_view4* q_out, const fasn_view4* k_new, const fasn_view4* v_new, char* buf, size_t cap);
int fasn_kvprefill_fp8_tree_rope_append_plan(const fasn_kvprefill_args* args, const fasn_kv_fp8* fp8, const fasn_kv_rope* rope, const fasn_kv_tree* tree,
                                             const fasn_view4* q_out, const fasn_view4* k_new, const fasn_view4* v_new, char* buf, size_t cap);
int fasn_kvcache_fp8_tree_commit(const fasn_kv_tree_commit* commit, fasn_stream_t stream);

/*
 * THE CACHE CALLS BY OPERAND SET (additions within ABI 6; no struct above is changed): the one host path below every named cache entry
 * point - argument block, then the operands present - as five entry points that take the operand set as data. A call is its block and
 * the non-NULL operand pointers; every named entry point above is one such call and keeps its name, its behaviour and its plan.
 *
 *   kind       which block `block` points at: FASN_KV_CALL_DECODE a fasn_kvcache_args, FASN_KV_CALL_PREFILL a fasn_kvprefill_args,
 *              FASN_KV_CALL_PACKED a fasn_kvvarlen_args. reserved = 0.
 *   operands   fp8, tree, window, alibi: NULL means "not part of the call". A forward reads all four. An append reads fp8, reads tree only
 *              when `rope` is given, and never reads window or alibi.
 *   checks     call == NULL, block == NULL, kind outside 0 .. 2 or reserved != 0 is FASN_EINVAL (fasn_kv_forward_workspace_bytes: 0).
 *              Everything else is the named calls' path: the block's rules first, then - a set without kernels is FASN_EUNSUPPORTED -
 *              the operands' rules in the family's one order (FP8, tree, window, ALiBi; a rotary append: as fasn_kv*_rope_append states).
 *              For a set a named entry point serves, the code, the workspace bytes and the plan text are that entry point's.
 *   forward    fasn_kv_forward_workspace_bytes / fasn_kv_forward / fasn_kv_forward_plan: fasn_fwd_kv*_workspace_bytes / fasn_fwd_kv* /
 *              fasn_kv*_plan of the set.
 *   append     fasn_kv_append: with `rope` the set's fasn_kv*_rope_append (q_out needed; k_new == v_new == NULL rotates the queries only),
 *              without it fasn_kv*_fp8_append when fp8 is given and fasn_kv*_append otherwise (q_out is not read). fasn_kv_append_plan
 *              writes its one launch as text.
 *
 * FP8 CACHE ON PACKED QUERIES. The sets a packed block has beside those of the named packed calls, reached through these entry points only:
 *   {fp8}, {fp8, window}   fasn_fwd_kvvarlen[_window] over the FP8 cache of fasn_fwd_kvprefill_fp8[_window]: the packed call's tokens,
 *              offsets, item table, outputs ([1, H, total_tokens, D] views, lse [H, total_tokens]), safety and - under a window - per-sequence
 *              memory contract, with the FP8 call's values; scale (b, hkv) is read at the token's sequence b. The launches are the schedule
 *              kernel, the forward and, with several splits, a combine kernel: grids, split count and workspace are those of the 16-bit
 *              packed call of the same shape (and window), the LDS is the FP8 prefill's. Checks: the block's, the packed operands', the
 *              FP8 operand's, the window's. D is 64 or 128.
 *   append     {fp8}: token t of k_new / v_new ([1, H / kv_group, total_tokens, D] views) quantised as fasn_kvprefill_fp8_append quantises
 *              a row, with the scales of its sequence, to cache row seqlens[b] + t - cu[b] under the rules of fasn_kvvarlen_append; one
 *              launch of ceil(total_tokens * (H / kv_group) * (D / 16) / 256) workgroups. {fp8} with `rope`: fasn_kvvarlen_rope_append in
 *              front of the FP8 cache - rotate, round once to `dtype`, quantise with k_scale, write the codes; v_new quantised beside it;
 *              the query token rotated into q_out - on that call's grid, as fasn_kvprefill_fp8_rope_append defines the values.
 * A packed block with a tree or with ALiBi slopes, and the FP8 cache with ALiBi slopes, are FASN_EUNSUPPORTED.
 */
enum { FASN_KV_CALL_DECODE = 0, FASN_KV_CALL_PREFILL = 1, FASN_KV_CALL_PACKED = 2 };
typedef struct fasn_kv_call {
    int32_t kind;                    /* FASN_KV_CALL_* */
    int32_t reserved;                /* 0 */
    const void* block;               /* fasn_kvcache_args / fasn_kvprefill_args / fasn_kvvarlen_args, by kind */
    const fasn_kv_fp8* fp8;          /* NULL: not part of the call */
    const fasn_kv_tree* tree;
    const fasn_kv_window* window;
    const fasn_alibi_slopes* alibi;
} fasn_kv_call;

size_t fasn_kv_forward_workspace_bytes(const fasn_kv_call* call);
int fasn_kv_forward(const fasn_kv_call* call, void* workspace, size_t workspace_bytes, fasn_stream_t stream);
int fasn_kv_forward_plan(const fasn_kv_call* call, char* buf, size_t cap);
int fasn_kv_append(const fasn_kv_call* call, const fasn_kv_rope* rope, const fasn_view4* q_out, const fasn_view4* k_new, const fasn_view4* v_new,
                   fasn_stream_t stream);
int fasn_kv_append_plan(const fasn_kv_call* call, const fasn_kv_rope* rope, const fasn_view4* q_out, const fasn_view4* k_new,
                        const fasn_view4* v_new, char* buf, size_t cap);

/*
 * DECODE BEHIND A SHARED PREFIX (additions within ABI 6; no struct or function above is changed): fasn_fwd_kvcache on a paged 16-bit cache
 * whose first P keys are the same physical pages for every batch element (a system prompt, a few-shot header, N samples of one prompt).
 * The prefix is walked once per K/V head for the rows of ALL batch elements, each batch element's own keys as fasn_fwd_kvcache walks them.
 *
 *   the virtual cache   P = clamp(*prefix_len, 0, min(max_prefix_pages * page_size, capacity)), read inside the kernels (never on the
 *              host: one captured graph serves every step and every prefix length). For every batch element b, key row j < P is row
 *              j % page_size of page prefix_table[j / page_size]; key row j >= P is the row block_table[b] names, as in fasn_fwd_kvcache.
 *              The result is exactly fasn_fwd_kvcache's on that cache: len_b, the positions p_i, what a row sees, softmax_n (counted
 *              once per row) and lse do not depend on P. A batch element with len_b < P sees prefix keys up to its own limit; P need
 *              not be a multiple of page_size or of 64 (a partially shared last page, copy on write).
 *   never read block_table[b] entries and the batch element's own cache rows for keys below P (slots wholly below P may be unset or
 *              point anywhere); prefix-page rows at or beyond P; prefix_table entries at or beyond ceil(P / page_size); rows at or
 *              beyond len_b. All of them may hold anything, NaN included.
 *   append     fasn_kvcache_append on the same block: k_new / v_new land in the batch element's OWN pages at seqlens[b] + i. Rows that
 *              land below P are never read.
 *   launches   three: the prefix pass - Hkv * ceil(B * R / 128) * nsplit_p workgroups of 256, R = kv_group * Sq, a workgroup holding
 *              128 rows of the row space b * R + r - the suffix pass - fasn_fwd_kvcache's grid B * Hkv * nsplit - and the combine,
 *              ceil(B * Hkv * R * (D / 4) / 256) workgroups. Grids, split counts and workspace depend on shapes, max_prefix_pages and
 *              capacity only.
 *   splits     nsplit is fasn_fwd_kvcache's for the block; split s of the suffix pass owns ceil((ceil(len_b / 64) - tlo) / nsplit) tiles
 *              from tlo = min(P / 64, ceil(len_b / 64)) on, the base call's ranges at P = 0. nsplit_p is the same rule over
 *              Hkv * ceil(B * R / 128) blocks and the ceil(min(max_prefix_pages * page_size, capacity) / 64) tiles a prefix can have, at
 *              least 16 tiles per split.
 *   workspace  (B * Hkv * nsplit * R + Hkv * nsplit_p * B * R) * (D + 2) * 4 bytes, 16-byte aligned.
 *   checks     the block's rules with fasn_fwd_kvcache's codes and order; then block_table == NULL (a dense cache) and D outside
 *              {64, 128}: FASN_EUNSUPPORTED; prefix == NULL, a NULL member, max_prefix_pages < 1 or reserved != 0: FASN_EINVAL; prefix_len
 *              or prefix_table not 4-byte aligned: FASN_EALIGN; then the workspace. args == NULL is FASN_EINVAL (workspace query: 0)
 *              before any HIP call. An FP8 cache, ALiBi, a window, a tree and packed queries have no shared-prefix kernels.
 */
typedef struct fasn_shared_prefix {
    const int32_t* prefix_len;     /* device, one int32 */
    const int32_t* prefix_table;   /* device, int32 [max_prefix_pages]: the page ids of the prefix, in order */
    int32_t max_prefix_pages;      /* >= 1 */
    int32_t reserved;              /* 0 */
} fasn_shared_prefix;

size_t fasn_fwd_shared_prefix_workspace_bytes(const fasn_kvcache_args* args, const fasn_shared_prefix* prefix);
int fasn_fwd_shared_prefix(const fasn_kvcache_args* args, const fasn_shared_prefix* prefix, void* workspace, size_t workspace_bytes, fasn_stream_t stream);
int fasn_shared_prefix_plan(const fasn_kvcache_args* args, const fasn_shared_prefix* prefix, char* buf, size_t cap);

/*
 * DECODE BEHIND SEVERAL SHARED PREFIXES: PREFIX GROUPS (additions within ABI 6; no struct or function above is changed): the call above
 * with one prefix per GROUP of batch elements - a server that holds a few system prompts, N samples of each of M prompts, sequences that
 * share nothing - in one launch set and one captured graph. Membership is device data: prefix_group[b] names the prefix of batch
 * element b, any value outside [0, num_groups) means "no shared prefix".
 *
 *   the virtual cache   for g = prefix_group[b] in [0, num_groups): P_b = clamp(prefix_lens[g], 0, min(max_prefix_pages * page_size,
 *              capacity)); key row j < P_b is row j % page_size of page prefix_tables[g * max_prefix_pages + j / page_size], key row
 *              j >= P_b the row block_table[b] names. For every other b, P_b = 0. The result is exactly fasn_fwd_kvcache's on that
 *              cache, as above: with every prefix_group entry out of range it is fasn_fwd_kvcache's bit for bit, with num_groups = 1
 *              and every entry 0 fasn_fwd_shared_prefix's.
 *   never read what fasn_fwd_shared_prefix never reads, per batch element and per group; and the prefix_tables row and every page of a
 *              group that has no member. Whatever prefix_group and prefix_lens hold, no access leaves the operands.
 *   append     fasn_kvcache_append on the same block, as above.
 *   launches   four: the schedule kernel (one workgroup of 256: prefix_group -> the table below), the prefix pass -
 *              Hkv * items_max * nsplit_p workgroups of 256, a workgroup holding one ITEM: 128 rows of one group - the suffix pass -
 *              fasn_fwd_kvcache's grid - and the combine. items_max = ceil(B * R / 128) + min(num_groups, B) - 1, R = kv_group * Sq.
 *              Grids, split counts and workspace depend on shapes, num_groups, max_prefix_pages and capacity only.
 *   splits     nsplit as above; nsplit_p is the same rule over Hkv * items_max blocks and the tiles a prefix can have, at least 16 tiles
 *              per split.
 *   workspace  partials of (B * Hkv * nsplit * R + Hkv * nsplit_p * B * R) * (D + 2) * 4 bytes, laid out as above; then, at the next
 *              multiple of 16 bytes - FASN_PREFIX_GROUPS_TABLE_OFFSET(partial bytes) - the schedule table of
 *              (4 + ceil(3 * B / 4) * 4 + 4 * items_max) int32. 16-byte aligned.
 *   the table  the grouped batch elements in a STABLE order - by group, inside a group by batch index - own the rows slot * R + r of the
 *              prefix partials. int32:
 *                [0] the item count, [1] the number of grouped batch elements, [2] [3] 0
 *                [4 + s]            order: the batch element of slot s; -1 at and beyond [1]            (s < B)
 *                [4 + B + b]        the slot of batch element b; -1: no prefix                            (b < B)
 *                [4 + 2 B + b]      P_b                                                                   (b < B)
 *                [4 + ceil(3 * B / 4) * 4 + 4 * i ..]  item i: group, first row, the row at which the group's rows end, P_g; a group
 *                                   of c members has ceil(c * R / 128) items of 128 rows from first row on; (-1, 0, 0, 0) at and beyond [0]
 *              Every entry is written by every call, and the same operands give the same table. It is output for inspection only.
 *   checks     the block's rules with fasn_fwd_kvcache's codes and order; then block_table == NULL and D outside {64, 128}:
 *              FASN_EUNSUPPORTED; groups == NULL, a NULL member, num_groups < 1 or > FASN_PREFIX_GROUPS_MAX, max_prefix_pages < 1 or
 *              reserved != 0: FASN_EINVAL; prefix_lens, prefix_tables or prefix_group not 4-byte aligned: FASN_EALIGN; then the workspace.
 */
#define FASN_PREFIX_GROUPS_MAX 1024   /* three LDS counters per group in the schedule kernel */
#define FASN_PREFIX_GROUPS_TABLE_OFFSET(partial_bytes) (((size_t)(partial_bytes) + 15) / 16 * 16)
typedef struct fasn_prefix_groups {
    const int32_t* prefix_lens;     /* device, int32 [num_groups] */
    const int32_t* prefix_tables;   /* device, int32 [num_groups][max_prefix_pages], contiguous: the page ids of prefix g, in order */
    const int32_t* prefix_group;    /* device, int32 [B]: the prefix of batch element b; outside [0, num_groups): none */
    int32_t num_groups;             /* 1 .. FASN_PREFIX_GROUPS_MAX */
    int32_t max_prefix_pages;       /* >= 1 */
    int32_t reserved;               /* 0 */
} fasn_prefix_groups;

size_t fasn_fwd_prefix_groups_workspace_bytes(const fasn_kvcache_args* args, const fasn_prefix_groups* groups);
int fasn_fwd_prefix_groups(const fasn_kvcache_args* args, const fasn_prefix_groups* groups, void* workspace, size_t workspace_bytes, fasn_stream_t stream);
int fasn_prefix_groups_plan(const fasn_kvcache_args* args, const fasn_prefix_groups* groups, char* buf, size_t cap);

/*
 * Stand-alone softmax_n over the last dimension of a [rows, cols] matrix (row stride in elements,
 * col stride 1). Replaces flash_attention_softmax_n/core/functional.py:15-29 for device tensors.
 * dtype: FASN_DTYPE_F16 / FASN_DTYPE_BF16 / 2 (= fp32).
 */
#define FASN_DTYPE_F32 2
int fasn_softmax_n_fwd(const void* x, void* y, int64_t rows, int64_t cols, int64_t x_row_stride,
                       int64_t y_row_stride, float n, int32_t dtype, fasn_stream_t stream);
/* dx = y * (dy - sum_j dy_j y_j)  (same formula as softmax; n only enters through y) */
int fasn_softmax_n_bwd(const void* y, const void* dy, void* dx, int64_t rows, int64_t cols,
                       int64_t y_row_stride, int64_t dy_row_stride, int64_t dx_row_stride,
                       int32_t dtype, fasn_stream_t stream);

/*
 * Power sums of every row of a [rows, cols] matrix in ONE pass (col stride 1, row stride in elements), taken about the row's
 * first element so that central moments formed from them do not cancel on data with a large offset:
 * sums[row][0..3] += sum d, sum d^2, sum d^3, sum d^4 with d = x - x[row][0] in fp64 (the caller zeroes `sums`). Replaces the repeated
 * mean / subtract / pow passes of flash_attention_softmax_n/analysis/statistics.py:9-79 (variance, skewness, kurtosis of
 * activations) for device tensors. dtype: FASN_DTYPE_F16 / BF16 / F32; rows <= 65535.
 */
int fasn_moments(const void* x, double* sums, int64_t rows, int64_t cols, int64_t row_stride, int32_t dtype,
                 fasn_stream_t stream);

/*
 * The one launch of the row kernels as text (ABI 6, in the line format of fasn_launch_plan): which kernel template, with which
 * arguments, on which grid. The plan calls ARE the calls above under the launch recorder: the same argument checks with the same
 * FASN_E* codes, the same selection function, no kernel run, no device touched, no HIP call made. Pointers only have to be
 * non-NULL; their alignment is read, since a pointer off 16 bytes sends a call to the element-load kernels. Return value as for
 * fasn_launch_plan: the bytes written, a FASN_E* code, or FASN_EINVAL when `cap` is too small.
 *
 * fasn_softmax_n_plan: `which` = FASN_ROW_FWD takes (a, b) = (x, y) and their row strides, c and c_row_stride are not read;
 * FASN_ROW_BWD takes (a, b, c) = (y, dy, dx). n is no argument: it does not enter the selection (a negative n is refused by the
 * forward alone). The kernels: softmax_n_{fwd,bwd}_wave_kernel<dtype, NV> (one wave per row, four rows per workgroup, NV 16-byte vectors
 * per lane), softmax_n_{fwd,bwd}_block_kernel<dtype, NV> (one workgroup per row, NV vectors per thread), and softmax_n_{fwd,bwd}_kernel<dtype>
 * (element loads: any alignment, any stride, any length).
 *
 * fasn_moments_plan: the arguments of fasn_moments; grid= is the number of chunks a row is cut into (grid.x; grid.y is `rows`).
 */
#define FASN_ROW_FWD 0
#define FASN_ROW_BWD 1
int fasn_softmax_n_plan(int32_t which, const void* a, const void* b, const void* c, int64_t rows, int64_t cols, int64_t a_row_stride,
                        int64_t b_row_stride, int64_t c_row_stride, int32_t dtype, char* buf, size_t cap);
int fasn_moments_plan(const void* x, const double* sums, int64_t rows, int64_t cols, int64_t row_stride, int32_t dtype, char* buf,
                      size_t cap);

/*
 * PACKED VARIABLE-LENGTH TRAINING ATTENTION (flash_attn_varlen_func for softmax_n; additions within ABI 6, the argument blocks above keep
 * their layouts): the sequences of a batch lie behind each other in one token buffer per side, and two tables of B + 1 int32 offsets in
 * DEVICE memory - cu[0] = 0, non-decreasing, cu[B] <= rows of the side - say where each sequence starts. Sequence b is fasn_fwd / fasn_bwd
 * on q[cu_q[b] : cu_q[b + 1]] against k, v[cu_k[b] : cu_k[b + 1]]: causal is bottom-right aligned per sequence (j <= i + sk_b - sq_b), a
 * row that sees no key gives 0 with lse = log n (-inf at n = 0) and zero gradients, a sequence may be empty on either side.
 *
 *   args      the forward / backward block describes the PACKED operands: B = 1, Sq / Sk = the token rows of the query / key side, every
 *             view [1, heads, rows, D] with stride[1] between heads, stride[2] between tokens, stride[0] unused; lse and delta
 *             [H, Sq] fp32 (lse must be given); kv_group as in fasn_fwd (dk / dv have H / kv_group heads, summed inside the kernel).
 *             dtype fp16 / bf16, D == Dv == 64. mask, bias and dbias NULL, dropout_p 0.
 *   varlen    cu_seqlens_q / cu_seqlens_k (the same pointer for self-attention), num_seqs = B >= 1, and max_seqlen_q / max_seqlen_k >= 1:
 *             host bounds of every length, constants of a captured graph. The grids are functions of num_seqs, max_seqlen_*, the heads
 *             and the rows alone; nothing is read on the host. A sequence longer than its bound is the caller's error: its rows beyond the
 *             bound are not computed. Whatever the tables hold, no kernel touches memory outside the operands: offsets are clamped to
 *             [0, rows] and made non-decreasing.
 *   n         NULL: args->softmax_n. Else a DEVICE fp32 value per query head, head h at n[h * n_stride_h] (stride 0: one value); an entry
 *             that is not > 0 acts as 0. Its gradient: fasn_bwd_dn on the [1, H, Sq] view of o, lse and dout.
 *   tail      rows at or beyond cu_q[B] come back as o = 0, lse = -inf, dq = 0; dk / dv rows at or beyond cu_k[B] as 0 (a small kernel of
 *             its own writes them); no byte between the rows of a strided view is written.
 *
 * fasn_fwd_varlen launches the tail kernel and the forward on num_seqs * H * ceil(max_seqlen_q / 128) workgroups; fasn_bwd_varlen the tail
 * kernel, the dQ kernel on the same grid (it publishes delta) and the dK/dV kernel on num_seqs * (H / kv_group) * ceil(max_seqlen_k / 128)
 * workgroups: deterministic, no atomics, no workspace. A workgroup reads its sequence's two offset pairs once and leaves at once when its
 * block lies beyond the sequence. fasn_varlen_plan writes the launches of the forward (FASN_PLAN_FWD) or the backward (FASN_PLAN_BWD) as
 * text, in the line format of fasn_launch_plan, with no HIP call.
 * Codes, checked in this order before any HIP call: a NULL block, NULL offsets, sizes < 1, B != 1, a bad enum, kv_group that does not
 * divide H, n_stride_h < 0 FASN_EINVAL; D != Dv FASN_EHEADDIM; fp32, a head dim other than 64, a mask, a bias, dropout or dbias
 * FASN_EUNSUPPORTED; then the views (FASN_EINVAL / FASN_ESTRIDE / FASN_EALIGN as in fasn_fwd, a side of 2^31 bytes or more FASN_EINVAL),
 * offsets or n off 4 bytes FASN_EALIGN.
 */
typedef struct fasn_varlen {
    const int32_t* cu_seqlens_q; /* DEVICE [num_seqs + 1] token offsets of the query side */
    const int32_t* cu_seqlens_k; /* DEVICE [num_seqs + 1] token offsets of the key / value side */
    int32_t num_seqs;
    int32_t max_seqlen_q;
    int32_t max_seqlen_k;
    int32_t reserved;            /* 0 */
} fasn_varlen;

int fasn_fwd_varlen(const fasn_fwd_args* args, const fasn_varlen* varlen, const float* n, int64_t n_stride_h, fasn_stream_t stream);
int fasn_bwd_varlen(const fasn_bwd_args* args, const fasn_varlen* varlen, fasn_stream_t stream);
int fasn_varlen_plan(const fasn_bwd_args* args, const fasn_varlen* varlen, int32_t which, char* buf, size_t cap);

/*
 * SLIDING WINDOW ON THE PACKED TRAINING CALL (additions within ABI 6; no struct is new: the operand is the cache calls' fasn_kv_window).
 * The positions are those of the cache calls: row i of sequence b sits at p_i = i + (sk_b - sq_b) and sees key j iff 0 <= j < sk_b and
 * p_i - window < j <= p_i - its own position counts, so `window` keys (the Hugging Face sliding_window rule). A row that sees no key gives
 * 0 with lse = log n (-inf at n = 0) and zero gradients. Everything else is the base call's: the tail rows, a device n, grouped K/V, strided
 * views, the grids - functions of num_seqs, max_seqlen_* and the heads; the window changes the walk inside a work item, not the items.
 *
 * fasn_fwd_varlen_window / fasn_bwd_varlen_window are fasn_fwd_varlen / fasn_bwd_varlen with the operand: the tail kernel, then forward / dQ
 * and dK/dV kernels of their own (the packed kernels compiled once more, under names of their own). fasn_varlen_window_plan is
 * fasn_varlen_plan for these launches. With window >= max_seqlen_k no key of any sequence can lie below a row's window: the three calls
 * then take the launches of the causal packed call - its plan text, its results bit for bit.
 * Codes: every rule and code of fasn_fwd_varlen / fasn_bwd_varlen holds and is checked first, in its order; then window == NULL,
 * window->window < 1 or reserved != 0 is FASN_EINVAL; then args->causal == 0 is FASN_EUNSUPPORTED (the window is causal, bottom-right
 * aligned). Any window >= 1 is legal.
 *
 * Memory contract (what "only the window's tiles" means). With coff_b = sk_b - sq_b, for the 128-row query block of sequence b that starts
 * at row q0, the forward and the dQ kernel read no K / V row of the sequence below 64 * floor(max(0, q0 + coff_b - window + 1) / 64): such
 * rows may hold anything. For a 128-key block, the dK/dV kernel uses no Q / dO / lse / delta row of a 64-row tile beyond tile
 * floor((last key of the block - coff_b + window - 1) / 64) (no tile at all when that is negative: dk / dv of the block are 0). A row that
 * a prefetch loads and no MFMA consumes is within the contract.
 */
int fasn_fwd_varlen_window(const fasn_fwd_args* args, const fasn_varlen* varlen, const fasn_kv_window* window, const float* n,
                           int64_t n_stride_h, fasn_stream_t stream);
int fasn_bwd_varlen_window(const fasn_bwd_args* args, const fasn_varlen* varlen, const fasn_kv_window* window, fasn_stream_t stream);
int fasn_varlen_window_plan(const fasn_bwd_args* args, const fasn_varlen* varlen, const fasn_kv_window* window, int32_t which, char* buf,
                            size_t cap);

/*
 * ROTARY POSITION EMBEDDING ON THE PACKED TRAINING CALL (additions within ABI 6; no struct is new: the operand is the cache calls'
 * fasn_kv_rope, with `rows` >= max_seqlen_k in the place of the capacity). ONE launch in front of fasn_fwd_varlen / fasn_fwd_varlen_window
 * that rotates the packed q and k rows at per-sequence positions, read from the two offset tables in device memory - a replayed graph
 * follows them. With [q0, q1) / [k0, k1) the token ranges of sequence b as the attention kernels clamp them, sq_b = q1 - q0, sk_b = k1 - k0:
 *   k       key token k0 + j, j < sk_b, of args->k is rotated at position j and written to the same row of k_out
 *   q       query token q0 + i, i < sq_b, of args->q is rotated at p_i = i + (sk_b - sq_b) - the p_i of the causal mask and of the window -
 *           and written to the same row of q_out. Self-attention: p_i = i; every sequence restarts at 0.
 * The table row read is clamp(pos, 0, rows - 1): the clamp acts on the negative p_i of rows that see no key. Layouts, tables and
 * rounding are those of the cache's rotary calls above (the kernels share the rotation's text): bit for bit (x1 c - x2 s), (x2 c + x1 s)
 * evaluated in fp32 step by step and rounded once. inverse = 1 applies the transpose rotation - the sines negated, which is exact:
 * y1 = x1 c + x2 s, y2 = x2 c - x1 s - and is what the backward applies to dq / dk where fasn_bwd_varlen left them.
 *
 *   args      the block of fasn_fwd_varlen; args->q and args->k are the SOURCES. v, o and lse are not touched and may be NULL here; every
 *             other member is checked as fasn_fwd_varlen checks it (one block serves both calls).
 *   q_out / k_out   [1, heads, rows, D] views under the rules of q / k. Each may be its source exactly (same pointer, same strides: in
 *             place); otherwise it must not overlap it.
 *   rows nobody owns - tokens at or beyond cu[B] of their side - are neither read nor written, and no byte between the rows of a strided
 *   view is written. Whatever the offset tables hold, no access leaves the operands and the tables.
 *
 * The launch runs ceil(Sq / 16) + ceil(Sk / 16) workgroups of 256 lanes - a function of the token rows alone, not of num_seqs or
 * max_seqlen_*, and never of the offsets. fasn_varlen_rope_plan writes it as text, in the line format of fasn_launch_plan, with no HIP call.
 * Codes, all before any HIP call: every rule and code of fasn_fwd_varlen that applies (all but those of v, o and lse), in its order;
 * then rope, cos, sin, q_out or k_out NULL, rotary_dim outside [16, D] or not a multiple of 16, rows < max_seqlen_k, interleaved not 0 or 1,
 * row_stride < rotary_dim / 2 FASN_EINVAL; table_dtype neither FASN_DTYPE_F32 nor args->dtype FASN_EDTYPE; a table base off 16 bytes or a
 * row stride that is no multiple of 16 bytes FASN_EALIGN; q_out, then k_out, with the codes of q; then inverse not 0 or 1 FASN_EINVAL.
 */
int fasn_varlen_rope(const fasn_fwd_args* args, const fasn_varlen* varlen, const fasn_kv_rope* rope, const fasn_view4* q_out,
                     const fasn_view4* k_out, int32_t inverse, fasn_stream_t stream);
int fasn_varlen_rope_plan(const fasn_fwd_args* args, const fasn_varlen* varlen, const fasn_kv_rope* rope, const fasn_view4* q_out,
                          const fasn_view4* k_out, int32_t inverse, char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* FASN_H_ */
