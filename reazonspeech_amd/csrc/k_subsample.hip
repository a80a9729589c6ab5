// k_subsample.hip — depthwise-striding x8 subsampling, the non-GEMM parts
// ([UPSTREAM] ConvSubsampling(dw_striding) with length masking after
// every conv).  Activations are channels-last ([B][T][F][C], C fastest) so that the pointwise
// convs are plain row-major GEMMs (k_gemm_bf16.hip) and the flatten before the output Linear is
// a no-op (the Linear's columns are permuted to (f, c) order at weight-prep time).
//
//   sub_conv0_dw1 : mel f32[B][T][80] -> conv0(1->C, k3 s2 p1) + ReLU + mask -> depthwise(k3 s2 p1)
//                   + bias + mask -> bf16 [B][T2][F2][C].  The conv0 activation ([B][C][T/2][40],
//                   2.9 GB in bf16 at B=256) is never written: each thread (= one channel) keeps a
//                   rolling 3x3 window of conv0 outputs in registers and the mel rows in LDS.
//   sub_dw        : bf16 [B][Tin][Fin][C] -> depthwise(k3 s2 p1) + bias + mask -> bf16 [B][Tout][Fout][C]
//   enc_lens      : per-utterance valid lengths after each of the three strided convs.
// sub_conv0_dw1 and sub_dw each have a first form (a workgroup per output row) and the default second form (a workgroup per run
// of output rows, *_run_kernel): the same arithmetic per element, the same bits; $RS_SUB_CONV0_OLD / $RS_SUB_DW_OLD select the
// first (tests/test_gpu_front_forms.py, profiles/pr_front_forms_ab.txt).
#include "rs_common.h"

namespace {

__global__ void enc_lens_kernel(const int32_t* __restrict__ n_frames, int B, int stages, int sub_kind, int32_t* __restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int n = n_frames[b];
    for (int s = 0; s < stages; ++s) {
        n = n > 0 ? (sub_kind ? (n >= 3 ? (n - 3) / 2 + 1 : 0) : (n + 2 - 3) / 2 + 1) : 0;      // rs_conv_len
        out[s * B + b] = n;
    }
}

__device__ __forceinline__ void put(uint16_t* p, float v) { *p = f32_to_bf16(v); }
__device__ __forceinline__ void put(float* p, float v) { *p = v; }

// grid (T2, B), block C threads (thread = channel); OT = uint16_t (bf16, the throughput mode) or float (parity mode)
template <typename OT>
__global__ __launch_bounds__(256) void sub_conv0_dw1_kernel(
    const float* __restrict__ feats, const int32_t* __restrict__ lens_stage /* [stages][B] */, int B, int t_max,
    int n_mels, int T2, int F1, int F2, int C, const float* __restrict__ w0 /* [9][C] */,
    const float* __restrict__ b0, const float* __restrict__ wd /* [9][C] */, const float* __restrict__ bd,
    OT* __restrict__ out) {
    const int b = blockIdx.y, t2 = blockIdx.x, c = threadIdx.x;
    const int L1 = lens_stage[0 * B + b], L2 = lens_stage[1 * B + b];
    OT* orow = out + (((size_t)b * T2 + t2) * F2) * C + c;
    if (t2 >= L2) {  // masked output row
        for (int f2 = 0; f2 < F2; ++f2) put(orow + (size_t)f2 * C, 0.0f);
        return;
    }
    float k0[9], kd[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) { k0[j] = w0[j * C + c]; kd[j] = wd[j * C + c]; }
    const float bias0 = b0[c], biasd = bd[c];
    const float* fb = feats + (size_t)b * t_max * n_mels;

    // The mel operand of every conv0 tap is the same for all 256 channels of the workgroup: its
    // address depends on (block, loop counter) only, so the row loads below are SCALAR loads
    // (s_load_dwordx4, 4 new mel bins of each of the 7 rows per output column) and the taps are v_fma
    // with an SGPR operand — no LDS staging and no LDS read per FMA (the LDS-broadcast version was
    // LDS-issue-bound at a quarter of the f32 VALU rate).  Zero padding costs nothing per tap: the
    // left mel bin -1 is the initial value of the carried column, out-of-range mel rows are read from
    // a clamped row with their taps' weights zeroed (kz), invalid conv0 rows are skipped (uniform).
    const float* rowp[7];
    bool rowok[7];
#pragma unroll
    for (int r = 0; r < 7; ++r) {
        const int tm = 4 * t2 - 3 + r;
        rowok[r] = tm >= 0 && tm < t_max;
        rowp[r] = fb + (size_t)(tm < 0 ? 0 : (tm >= t_max ? t_max - 1 : tm)) * n_mels;
    }
    float kz[3][9];
    bool a_ok[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int t1 = 2 * t2 - 1 + a;
        a_ok[a] = t1 >= 0 && t1 < L1;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) kz[a][i * 3 + j] = rowok[2 * a + i] ? k0[i * 3 + j] : 0.0f;
    }
    float carry[7];
#pragma unroll
    for (int r = 0; r < 7; ++r) carry[r] = 0.0f;     // mel bin -1
    float left[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) left[a] = 0.0f;      // f1 = -1 is padding
    for (int f2 = 0; f2 < F2; ++f2) {
        float m[7][5];                               // mel bins 4*f2-1 .. 4*f2+3 of the 7 rows
#pragma unroll
        for (int r = 0; r < 7; ++r) {
            const float4 q = *reinterpret_cast<const float4*>(rowp[r] + 4 * f2);
            m[r][0] = carry[r]; m[r][1] = q.x; m[r][2] = q.y; m[r][3] = q.z; m[r][4] = q.w;
            carry[r] = q.w;
        }
        float mid[3], right[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            float am = 0.0f, ar = 0.0f;
            if (a_ok[a]) {
                am = bias0; ar = bias0;
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        am = fmaf(kz[a][i * 3 + j], m[2 * a + i][j], am);          // f1 = 2*f2   : bins 4*f2-1 .. 4*f2+1
                        ar = fmaf(kz[a][i * 3 + j], m[2 * a + i][2 + j], ar);      // f1 = 2*f2+1 : bins 4*f2+1 .. 4*f2+3
                    }
                am = fmaxf(am, 0.0f); ar = fmaxf(ar, 0.0f);
            }
            mid[a] = am; right[a] = ar;
        }
        float acc = biasd;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            acc = fmaf(kd[a * 3 + 0], left[a], acc);
            acc = fmaf(kd[a * 3 + 1], mid[a], acc);
            acc = fmaf(kd[a * 3 + 2], right[a], acc);
        }
        put(orow + (size_t)f2 * C, acc);
#pragma unroll
        for (int a = 0; a < 3; ++a) left[a] = right[a];
    }
}

// The same operator, a workgroup per RUN of SUB_RUN consecutive output rows of one utterance: grid (ceil(T2 / SUB_RUN), B),
// block C / 2 threads.  Conv0 row t1 = 2 t2 + 1 is the bottom row (a = 2) of output row t2 and the top row (a = 0) of t2 + 1; the
// kernel above computes it in both workgroups (54 conv0 FMAs per output where 36 are needed).  Here its ReLU'd values of all F2C
// columns (cm / cr: f1 = 2 f2 and 2 f2 + 1) stay in registers for the next row of the run, so only the first row of a run
// computes its top row (18 / (45 SUB_RUN) extra).  The carried values have the bits of the recomputed ones: bias0 plus the same
// nine fmaf in the same order on mel rows tm = 2 t1 - 1 + i with the same clamp and zeroed taps, and a_ok depends on t1 alone.
// F2C is a template argument because the column loop must be unrolled for cm / cr to be registers.
constexpr int SUB_RUN = 12;

// A thread owns two adjacent channels (V = two floats), so every pair of fmaf is one packed v_pk_fma_f32 — each half a fused
// multiply-add of its own: the same bits — with the mel value, a scalar register, as the operand of both halves; the
// one-channel-per-thread version of this kernel measured 14 us slower (profiles/pr_front_forms_ab.txt).
typedef float f32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2_t vfma(f32x2_t a, f32x2_t b, f32x2_t c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f32x2_t vfma(f32x2_t a, float b, f32x2_t c) { const f32x2_t bb = {b, b}; return __builtin_elementwise_fma(a, bb, c); }
__device__ __forceinline__ f32x2_t vrelu(f32x2_t a) { const f32x2_t r = {fmaxf(a.x, 0.0f), fmaxf(a.y, 0.0f)}; return r; }
__device__ __forceinline__ void vload(const float* p, f32x2_t& v) { v = *reinterpret_cast<const f32x2_t*>(p); }
__device__ __forceinline__ void put(uint16_t* p, f32x2_t v) {
    const unsigned u = (unsigned)f32_to_bf16(v.x) | ((unsigned)f32_to_bf16(v.y) << 16);
    *reinterpret_cast<unsigned*>(p) = u;
}
__device__ __forceinline__ void put(float* p, f32x2_t v) { *reinterpret_cast<f32x2_t*>(p) = v; }

template <typename OT, int F2C>
__global__ __launch_bounds__(256) void sub_conv0_dw1_run_kernel(
    const float* __restrict__ feats, const int32_t* __restrict__ lens_stage /* [stages][B] */, int B, int t_max,
    int n_mels, int T2, int C, const float* __restrict__ w0 /* [9][C] */, const float* __restrict__ b0,
    const float* __restrict__ wd /* [9][C] */, const float* __restrict__ bd, OT* __restrict__ out) {
    using V = f32x2_t;
    const int b = blockIdx.y, t2_first = blockIdx.x * SUB_RUN, c = threadIdx.x * 2;
    const int L1 = lens_stage[0 * B + b], L2 = lens_stage[1 * B + b];
    const int t2_end = min(t2_first + SUB_RUN, T2);
    const int t2_live = min(t2_end, L2);             // rows [t2_first, t2_live) are computed, [.., t2_end) are masked
    OT* obase = out + ((size_t)b * T2 * F2C) * C + c;
    const V zero = {};
    if (t2_first < t2_live) {
        V k0[9], kd[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) { vload(w0 + j * C + c, k0[j]); vload(wd + j * C + c, kd[j]); }
        V bias0, biasd;
        vload(b0 + c, bias0); vload(bd + c, biasd);
        const float* fb = feats + (size_t)b * t_max * n_mels;
        // The scalar loads of a row's mel bins miss the scalar cache once per 64 bytes, and the features were written by the
        // kernel before: a miss that goes to HBM stalls the wave for longer than the other waves of the SIMD can cover.  So the
        // first lanes touch the NEXT output row's five mel rows (5 * 320 bytes) with one vector load each, a row ahead: the
        // scalar misses then end in L2.  The loaded values are summed into `touched`, which is never stored.
        float touched = 0.0f;
        auto touch = [&](int tm_first) -> float {
            const int at = tm_first * n_mels + (int)threadIdx.x * 16;
            return (int)threadIdx.x * 16 < 5 * n_mels ? fb[min(max(at, 0), t_max * n_mels - 1)] : 0.0f;
        };
        const float touched_first = touch(4 * t2_first - 1);
        V cm[F2C], cr[F2C];
        {   // conv0 row t1 = 2 t2_first - 1 of every column: what the run above would have handed over
            const int t1 = 2 * t2_first - 1;
#pragma unroll
            for (int f2 = 0; f2 < F2C; ++f2) { cm[f2] = zero; cr[f2] = zero; }
            if (t1 >= 0 && t1 < L1) {                // (uniform)
                const float* rowp[3];
                V kz[9];
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const int tm = 2 * t1 - 1 + i;
                    const bool ok = tm >= 0 && tm < t_max;
                    rowp[i] = fb + (size_t)(tm < 0 ? 0 : (tm >= t_max ? t_max - 1 : tm)) * n_mels;
#pragma unroll
                    for (int j = 0; j < 3; ++j) kz[i * 3 + j] = ok ? k0[i * 3 + j] : zero;
                }
                float carry[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int f2 = 0; f2 < F2C; ++f2) {
                    float m[3][5];
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        const float4 q = *reinterpret_cast<const float4*>(rowp[i] + 4 * f2);
                        m[i][0] = carry[i]; m[i][1] = q.x; m[i][2] = q.y; m[i][3] = q.z; m[i][4] = q.w;
                        carry[i] = q.w;
                    }
                    V am = bias0, ar = bias0;
#pragma unroll
                    for (int i = 0; i < 3; ++i)
#pragma unroll
                        for (int j = 0; j < 3; ++j) {
                            am = vfma(kz[i * 3 + j], m[i][j], am);
                            ar = vfma(kz[i * 3 + j], m[i][2 + j], ar);
                        }
                    cm[f2] = vrelu(am); cr[f2] = vrelu(ar);
                }
            }
        }
        for (int t2 = t2_first; t2 < t2_live; ++t2) {
            // mel rows 4 t2 - 1 .. 4 t2 + 3 (r = 2 .. 6 of the kernel above) feed conv0 rows a = 1, 2
            const float touched_next = touch(4 * t2 + 3);
            const float* rowp[5];
            bool rowok[5];
#pragma unroll
            for (int r = 0; r < 5; ++r) {
                const int tm = 4 * t2 - 1 + r;
                rowok[r] = tm >= 0 && tm < t_max;
                rowp[r] = fb + (size_t)(tm < 0 ? 0 : (tm >= t_max ? t_max - 1 : tm)) * n_mels;
            }
            V kz[2][9];
            bool a_ok[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const int t1 = 2 * t2 + a;
                a_ok[a] = t1 >= 0 && t1 < L1;
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j) kz[a][i * 3 + j] = rowok[2 * a + i] ? k0[i * 3 + j] : zero;
            }
            float carry[5];
#pragma unroll
            for (int r = 0; r < 5; ++r) carry[r] = 0.0f;     // mel bin -1
            V left[3] = {zero, zero, zero};                  // f1 = -1 is padding
            OT* orow = obase + ((size_t)t2 * F2C) * C;
#pragma unroll
            for (int f2 = 0; f2 < F2C; ++f2) {
                float m[5][5];
#pragma unroll
                for (int r = 0; r < 5; ++r) {
                    const float4 q = *reinterpret_cast<const float4*>(rowp[r] + 4 * f2);
                    m[r][0] = carry[r]; m[r][1] = q.x; m[r][2] = q.y; m[r][3] = q.z; m[r][4] = q.w;
                    carry[r] = q.w;
                }
                V mid[3], right[3];
                mid[0] = cm[f2]; right[0] = cr[f2];
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    V am = zero, ar = zero;
                    if (a_ok[a]) {
                        am = bias0; ar = bias0;
#pragma unroll
                        for (int i = 0; i < 3; ++i)
#pragma unroll
                            for (int j = 0; j < 3; ++j) {
                                am = vfma(kz[a][i * 3 + j], m[2 * a + i][j], am);
                                ar = vfma(kz[a][i * 3 + j], m[2 * a + i][2 + j], ar);
                            }
                        am = vrelu(am); ar = vrelu(ar);
                    }
                    mid[a + 1] = am; right[a + 1] = ar;
                }
                V acc = biasd;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    acc = vfma(kd[a * 3 + 0], left[a], acc);
                    acc = vfma(kd[a * 3 + 1], mid[a], acc);
                    acc = vfma(kd[a * 3 + 2], right[a], acc);
                }
                put(orow + (size_t)f2 * C, acc);
#pragma unroll
                for (int a = 0; a < 3; ++a) left[a] = right[a];
                cm[f2] = mid[2]; cr[f2] = right[2];          // the bottom row is the next row's top row
            }
            touched += touched_next;
        }
        if (touched + touched_first == 1.0e-30f && t_max < 0) put(obase, zero);      // (never: keeps the touching loads)
    }
    for (int t2 = max(t2_first, t2_live); t2 < t2_end; ++t2) {   // masked output rows
        OT* orow = obase + ((size_t)t2 * F2C) * C;
        for (int f2 = 0; f2 < F2C; ++f2) put(orow + (size_t)f2 * C, zero);
    }
}

// grid (ceil(Fout / fpb), Tout, B); block 256 = (C/8 channel groups) x fpb
__global__ __launch_bounds__(256) void sub_dw_kernel(const uint16_t* __restrict__ in, const float* __restrict__ w /* [9][C] */,
                                                     const float* __restrict__ bias, const int32_t* __restrict__ lens_out,
                                                     int Tin, int Fin, int Tout, int Fout, int C,
                                                     uint16_t* __restrict__ out) {
    const int cgs = C >> 3;
    const int cg = threadIdx.x % cgs, fl = threadIdx.x / cgs, fpb = blockDim.x / cgs;
    const int fo = blockIdx.x * fpb + fl, to = blockIdx.y, b = blockIdx.z;
    if (fo >= Fout) return;
    const int c = cg * 8;
    uint16_t* op = out + (((size_t)b * Tout + to) * Fout + fo) * C + c;
    u16x8_t o;
    if (to >= lens_out[b]) {
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = 0;
        *reinterpret_cast<u16x8_t*>(op) = o;
        return;
    }
    float acc[8];
    {
        const float4 b0 = reinterpret_cast<const float4*>(bias + c)[0], b1 = reinterpret_cast<const float4*>(bias + c)[1];
        acc[0] = b0.x; acc[1] = b0.y; acc[2] = b0.z; acc[3] = b0.w; acc[4] = b1.x; acc[5] = b1.y; acc[6] = b1.z; acc[7] = b1.w;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int ti = 2 * to - 1 + i;
        if (ti < 0 || ti >= Tin) continue;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int fi = 2 * fo - 1 + j;
            if (fi < 0 || fi >= Fin) continue;
            const u16x8_t x = *reinterpret_cast<const u16x8_t*>(in + (((size_t)b * Tin + ti) * Fin + fi) * C + c);
            const float4 w0 = reinterpret_cast<const float4*>(w + (i * 3 + j) * C + c)[0];
            const float4 w1 = reinterpret_cast<const float4*>(w + (i * 3 + j) * C + c)[1];
            acc[0] = fmaf(w0.x, bf16_to_f32(x[0]), acc[0]); acc[1] = fmaf(w0.y, bf16_to_f32(x[1]), acc[1]);
            acc[2] = fmaf(w0.z, bf16_to_f32(x[2]), acc[2]); acc[3] = fmaf(w0.w, bf16_to_f32(x[3]), acc[3]);
            acc[4] = fmaf(w1.x, bf16_to_f32(x[4]), acc[4]); acc[5] = fmaf(w1.y, bf16_to_f32(x[5]), acc[5]);
            acc[6] = fmaf(w1.z, bf16_to_f32(x[6]), acc[6]); acc[7] = fmaf(w1.w, bf16_to_f32(x[7]), acc[7]);
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = f32_to_bf16(acc[e]);
    *reinterpret_cast<u16x8_t*>(op) = o;
}

// The same operator, a workgroup per RUN of DW_RUN consecutive output rows of one utterance: grid (ceil(Tout / DW_RUN), B),
// block (C / 8) * Fout threads, thread = (output bin, 8 channels) for every row of the run — every thread slot works at any C.
// The 72 weights and the bias are read once per run, not once per output; input row 2 to + 1 serves outputs to and to + 1 and
// is held in registers in between, so a run reads 2 DW_RUN + 1 input rows, each once.  Accumulation as above: bias, then the
// taps i outer, j inner, an out-of-range tap skipped.
constexpr int DW_RUN = 6;

__device__ __forceinline__ void dw_taps(float (&acc)[8], const float (&wt)[9][8], int i, const u16x8_t (&x)[3], const bool (&jok)[3]) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        if (!jok[j]) continue;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = fmaf(wt[i * 3 + j][e], bf16_to_f32(x[j][e]), acc[e]);
    }
}

__global__ __launch_bounds__(512) void sub_dw_run_kernel(const uint16_t* __restrict__ in, const float* __restrict__ w /* [9][C] */,
                                                         const float* __restrict__ bias, const int32_t* __restrict__ lens_out,
                                                         int Tin, int Fin, int Tout, int Fout, int C,
                                                         uint16_t* __restrict__ out) {
    const int cgs = C >> 3;
    const int cg = threadIdx.x % cgs, fo = threadIdx.x / cgs;     // fo < Fout: the block has cgs * Fout threads
    const int b = blockIdx.y, to_first = blockIdx.x * DW_RUN;
    const int c = cg * 8;
    const int to_end = min(to_first + DW_RUN, Tout);
    const int to_live = min(to_end, lens_out[b]);                 // rows [to_first, to_live) are computed, [.., to_end) are masked
    uint16_t* obase = out + (((size_t)b * Tout) * Fout + fo) * C + c;
    if (to_first < to_live) {
        float wt[9][8], bs[8];
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const float4 w0 = reinterpret_cast<const float4*>(w + k * C + c)[0], w1 = reinterpret_cast<const float4*>(w + k * C + c)[1];
            wt[k][0] = w0.x; wt[k][1] = w0.y; wt[k][2] = w0.z; wt[k][3] = w0.w; wt[k][4] = w1.x; wt[k][5] = w1.y; wt[k][6] = w1.z; wt[k][7] = w1.w;
        }
        {
            const float4 b0 = reinterpret_cast<const float4*>(bias + c)[0], b1 = reinterpret_cast<const float4*>(bias + c)[1];
            bs[0] = b0.x; bs[1] = b0.y; bs[2] = b0.z; bs[3] = b0.w; bs[4] = b1.x; bs[5] = b1.y; bs[6] = b1.z; bs[7] = b1.w;
        }
        bool jok[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) { const int fi = 2 * fo - 1 + j; jok[j] = fi >= 0 && fi < Fin; }
        const uint16_t* ibase = in + ((size_t)b * Tin * Fin) * C + c;
        // input row ti, bins 2 fo - 1 .. 2 fo + 1 of this thread's 8 channels (a bin outside the row is not read)
        auto load_row = [&](int ti, u16x8_t (&x)[3]) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                if (jok[j]) x[j] = *reinterpret_cast<const u16x8_t*>(ibase + ((size_t)ti * Fin + (2 * fo - 1 + j)) * C);
                else
#pragma unroll
                    for (int e = 0; e < 8; ++e) x[j][e] = 0;
            }
        };
        u16x8_t top[3], mid[3], bot[3];
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int e = 0; e < 8; ++e) { top[j][e] = 0; mid[j][e] = 0; bot[j][e] = 0; }
        bool top_ok = to_first > 0 && 2 * to_first - 1 < Tin;
        if (top_ok) load_row(2 * to_first - 1, top);
        // the two new rows of output row `to` are asked for one output row ahead, so that a wave has memory requests in
        // flight while it computes (the input was just written by the GEMM in front: it comes from HBM)
        u16x8_t mid_next[3], bot_next[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) { mid_next[j] = mid[j]; bot_next[j] = bot[j]; }
        if (2 * to_first < Tin) load_row(2 * to_first, mid_next);
        if (2 * to_first + 1 < Tin) load_row(2 * to_first + 1, bot_next);
        for (int to = to_first; to < to_live; ++to) {
            const bool mid_ok = 2 * to < Tin, bot_ok = 2 * to + 1 < Tin;      // (uniform)
#pragma unroll
            for (int j = 0; j < 3; ++j) { mid[j] = mid_next[j]; bot[j] = bot_next[j]; }
            if (to + 1 < to_live) {
                if (2 * to + 2 < Tin) load_row(2 * to + 2, mid_next);
                if (2 * to + 3 < Tin) load_row(2 * to + 3, bot_next);
            }
            float acc[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = bs[e];
            if (top_ok) dw_taps(acc, wt, 0, top, jok);
            if (mid_ok) dw_taps(acc, wt, 1, mid, jok);
            if (bot_ok) dw_taps(acc, wt, 2, bot, jok);
            u16x8_t o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = f32_to_bf16(acc[e]);
            *reinterpret_cast<u16x8_t*>(obase + ((size_t)to * Fout) * C) = o;
#pragma unroll
            for (int j = 0; j < 3; ++j) top[j] = bot[j];
            top_ok = bot_ok;
        }
    }
    u16x8_t z;
#pragma unroll
    for (int e = 0; e < 8; ++e) z[e] = 0;
    for (int to = max(to_first, to_live); to < to_end; ++to) *reinterpret_cast<u16x8_t*>(obase + ((size_t)to * Fout) * C) = z;
}

// the same depthwise conv on float32 activations (parity mode): one thread per output element, channel fastest
__global__ __launch_bounds__(256) void sub_dw_f32_kernel(const float* __restrict__ in, const float* __restrict__ w /* [9][C] */,
                                                         const float* __restrict__ bias, const int32_t* __restrict__ lens_out,
                                                         int Tin, int Fin, int Tout, int Fout, int C, float* __restrict__ out) {
    const int c = threadIdx.x, fo = blockIdx.x, to = blockIdx.y, b = blockIdx.z;
    float* op = out + (((size_t)b * Tout + to) * Fout + fo) * C + c;
    if (to >= lens_out[b]) { *op = 0.0f; return; }
    float acc = bias[c];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int ti = 2 * to - 1 + i;
        if (ti < 0 || ti >= Tin) continue;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int fi = 2 * fo - 1 + j;
            if (fi < 0 || fi >= Fin) continue;
            acc = fmaf(w[(i * 3 + j) * C + c], in[(((size_t)b * Tin + ti) * Fin + fi) * C + c], acc);
        }
    }
    *op = acc;
}

}  // namespace

int rs_launch_enc_lens(rs_ctx* ctx, const int32_t* n_frames, int B, int32_t* lens_out, hipStream_t s) {
    hipLaunchKernelGGL(enc_lens_kernel, dim3((B + 127) / 128), dim3(128), 0, s, n_frames, B, ctx->d.sub_stages, ctx->d.sub_kind, lens_out);
    RS_CHECK_LAUNCH(ctx, "enc_lens");
    return RS_OK;
}

// The run form is built for the 20 output columns of 80 mel bins (every shipped configuration); another width runs the first form.
constexpr int SUB_F2 = 20;
static bool conv0_run_form(int F2) { return F2 == SUB_F2 && !rs_knob(RS_KNOB_SUB_CONV0_OLD); }

int rs_launch_sub_conv0_dw1(rs_ctx* ctx, const float* feats, const int32_t* lens_stage, int B, int t_max, int T2,
                            int F2, uint16_t* out, hipStream_t s) {
    const rs_dims& d = ctx->d;
    const rs_conformer& cf = *rs_conformer_of(ctx);
    const int C = d.sub_channels;
    if (C > 256 || (C % 64)) return rs_fail(ctx, RS_EINVAL, "subsampling: channels %d unsupported (<=256, %%64)", C);
    const int F1 = (d.n_mels + 2 - 3) / 2 + 1;
    if (d.n_mels % 4 || 4 * F2 > d.n_mels || 2 * F2 < F1)
        return rs_fail(ctx, RS_EINVAL, "subsampling: n_mels=%d must be a multiple of 4 with 4*F2 <= n_mels", d.n_mels);
    const size_t lds = 0;
    const double flops = (double)B * T2 * F2 * C * 2.0 * (6 * 9 + 9);
    const double bytes = (double)B * t_max * d.n_mels * 4.0 + (double)B * T2 * F2 * C * 2.0;
    rs_prof_scope prof(ctx, RS_PROF_SUBSAMPLE, s, flops, bytes);
    if (conv0_run_form(F2))
        hipLaunchKernelGGL((sub_conv0_dw1_run_kernel<uint16_t, SUB_F2>), dim3((T2 + SUB_RUN - 1) / SUB_RUN, B), dim3(C / 2), lds, s, feats,
                           lens_stage, B, t_max, d.n_mels, T2, C, cf.sub_conv0_w, cf.sub_conv0_b, cf.sub_dw_w[0], cf.sub_dw_b[0], out);
    else
        hipLaunchKernelGGL(sub_conv0_dw1_kernel<uint16_t>, dim3(T2, B), dim3(C), lds, s, feats, lens_stage, B, t_max, d.n_mels, T2,
                       F1, F2, C, cf.sub_conv0_w, cf.sub_conv0_b, cf.sub_dw_w[0], cf.sub_dw_b[0], out);
    prof.end();
    RS_CHECK_LAUNCH(ctx, "sub_conv0_dw1");
    return RS_OK;
}

int rs_launch_sub_dw(rs_ctx* ctx, const uint16_t* in, const float* w, const float* b, const int32_t* lens_out,
                     int stage, int B, int t_in, int f_in, int t_out, int f_out, uint16_t* out, hipStream_t s) {
    (void)stage;
    const int C = ctx->d.sub_channels;
    const int cgs = C / 8;
    const int fpb = 256 / cgs;
    const dim3 grid((f_out + fpb - 1) / fpb, t_out, B), block(cgs * fpb);
    const double bytes = (double)B * C * 2.0 * ((double)t_in * f_in + (double)t_out * f_out);
    rs_prof_scope prof(ctx, RS_PROF_SUBSAMPLE, s, (double)B * t_out * f_out * C * 18.0, bytes);
    if (!rs_knob(RS_KNOB_SUB_DW_OLD) && cgs * f_out <= 512)      // (C <= 256, n_mels <= 128: at most 32 * 16 threads)
        hipLaunchKernelGGL(sub_dw_run_kernel, dim3((t_out + DW_RUN - 1) / DW_RUN, B), dim3(cgs * f_out), 0, s, in, w, b, lens_out, t_in,
                           f_in, t_out, f_out, C, out);
    else
        hipLaunchKernelGGL(sub_dw_kernel, grid, block, 0, s, in, w, b, lens_out, t_in, f_in, t_out, f_out, C, out);
    prof.end();
    RS_CHECK_LAUNCH(ctx, "sub_dw");
    return RS_OK;
}

// ---- float32 parity mode (k_f32.hip): the same two operators storing / reading float32 activations ----------------
int rs_launch_sub_conv0_dw1_f32(rs_ctx* ctx, const float* feats, const int32_t* lens_stage, int B, int t_max, int T2, int F2,
                                float* out, hipStream_t s) {
    const rs_dims& d = ctx->d;
    const rs_conformer& cf = *rs_conformer_of(ctx);
    const int C = d.sub_channels;
    if (C > 256 || (C % 64)) return rs_fail(ctx, RS_EINVAL, "subsampling: channels %d unsupported (<=256, %%64)", C);
    const int F1 = (d.n_mels + 2 - 3) / 2 + 1;
    if (d.n_mels % 4 || 4 * F2 > d.n_mels || 2 * F2 < F1)
        return rs_fail(ctx, RS_EINVAL, "subsampling: n_mels=%d must be a multiple of 4 with 4*F2 <= n_mels", d.n_mels);
    rs_prof_scope prof(ctx, RS_PROF_SUBSAMPLE, s, (double)B * T2 * F2 * C * 2.0 * (6 * 9 + 9),
                       (double)B * t_max * d.n_mels * 4.0 + (double)B * T2 * F2 * C * 4.0);
    if (conv0_run_form(F2))
        hipLaunchKernelGGL((sub_conv0_dw1_run_kernel<float, SUB_F2>), dim3((T2 + SUB_RUN - 1) / SUB_RUN, B), dim3(C / 2), 0, s, feats,
                           lens_stage, B, t_max, d.n_mels, T2, C, cf.sub_conv0_w, cf.sub_conv0_b, cf.sub_dw_w[0], cf.sub_dw_b[0], out);
    else
        hipLaunchKernelGGL(sub_conv0_dw1_kernel<float>, dim3(T2, B), dim3(C), 0, s, feats, lens_stage, B, t_max, d.n_mels, T2, F1, F2, C,
                       cf.sub_conv0_w, cf.sub_conv0_b, cf.sub_dw_w[0], cf.sub_dw_b[0], out);
    prof.end();
    RS_CHECK_LAUNCH(ctx, "sub_conv0_dw1_f32");
    return RS_OK;
}

int rs_launch_sub_dw_f32(rs_ctx* ctx, const float* in, const float* w, const float* b, const int32_t* lens_out, int B, int t_in,
                         int f_in, int t_out, int f_out, float* out, hipStream_t s) {
    const int C = ctx->d.sub_channels;
    rs_prof_scope prof(ctx, RS_PROF_SUBSAMPLE, s, (double)B * t_out * f_out * C * 18.0,
                       (double)B * C * 4.0 * ((double)t_in * f_in + (double)t_out * f_out));
    hipLaunchKernelGGL(sub_dw_f32_kernel, dim3(f_out, t_out, B), dim3(C), 0, s, in, w, b, lens_out, t_in, f_in, t_out, f_out, C, out);
    prof.end();
    RS_CHECK_LAUNCH(ctx, "sub_dw_f32");
    return RS_OK;
}
