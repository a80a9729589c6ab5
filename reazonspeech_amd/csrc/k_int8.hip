// k_int8.hip — onnxruntime's dynamically quantized MatMul on the int8 matrix cores (the "int8" / "int8-fp32" ONNX files of
// `reazonspeech.k2.asr`; rs_set_option "precision_i8").
//
// [UPSTREAM] onnxruntime.quantization.quantize_dynamic(op_types_to_quantize=["MatMul"], weight_type=QInt8) rewrites a MatMul
// whose B operand is a constant into
//     DynamicQuantizeLinear(x) -> (xq uint8, sx, zx);  MatMulInteger(xq, Wq int8 [K][N], zx, zw) -> int32;  Cast -> float;
//     Mul(., Mul(sx, sw));  + the bias Add of the float graph
// with ONE scale and zero point per TENSOR (the ONNX spec of DynamicQuantizeLinear):
//     sx = (max(0, max x) - min(0, min x)) / 255   (onnxruntime: 1 when that range is empty),
//     zx = saturate(round(-min(0, min x) / sx)),  xq = saturate(round(x / sx) + zx),  round = half to even, saturate = [0, 255].
// sherpa-onnx runs one utterance per call, so "per tensor" is per utterance here: the rows of a launch come in groups of
// `group` rows, one group per utterance, and only the first lens[g] rows of a group enter its statistics.
//
//   i8_range_kernel    (sx, zx) per group: min / max over its valid rows (order-independent, so deterministic), one block a group
//   gemm_i8q_kernel    out = epilogue(float(sum_k (xq - zx)(Wq - zw)) * fl(sx sw) + bias): A arrives as float32 and is quantized
//                      while it is loaded (x / sx correctly rounded: v_div_scale / v_div_fmas / v_div_fixup, no v_rcp), the
//                      products run on v_mfma_i32_16x16x64_i8 with the signed operand a = xq - 128, and the zero points are
//                      restored exactly from the weights' column sums cs[n] = sum_k Wq[n][k] (and the row sums of a when zw != 0):
//                          sum (xq - zx)(Wq - zw) = sum a Wq + (128 - zx) cs - zw (sum a + K (128 - zx))
//                      all in int32 (|.| <= 255 * 255 * K + ...: far below 2^31 for the model's K).  The weights stay int8 in HBM.
// Compiled with -ffp-contract=off (build.py EXTRA): the epilogue is the graph's own sequence of float32 roundings — the Cast,
// the Mul, the bias Add, then the float graph's Swoosh / residual Add.
#include "rs_common.h"

namespace {

typedef int i32x4_t __attribute__((ext_vector_type(4)));

constexpr int IBM = 64, IBN = 128, IBK = 64, ILD = IBK + 16;     // tile rows (activations), rows (weights), k step; LDS row pitch in bytes

__device__ __forceinline__ float quant_u8(float x, float sx, float zx) {
    const float q = rintf(__fdiv_rn(x, sx)) + zx;
    return fminf(fmaxf(q, 0.0f), 255.0f);                 // (a NaN input lands on 0)
}

// grid (groups), block 1024: qp[g] = (sx, zx) of the first min(lens[g], group) rows of group g, columns < K
__global__ __launch_bounds__(1024) void i8_range_kernel(const float* __restrict__ A, int lda, const int32_t* __restrict__ lens, int group, int K,
                                                        float* __restrict__ qp) {
    const int g = blockIdx.x;
    int rows = lens[g];
    rows = rows < 0 ? 0 : (rows > group ? group : rows);
    const float* base = A + (size_t)g * group * lda;
    float mn = 0.0f, mx = 0.0f;                           // min(0, .) / max(0, .): the range always holds zero
    if ((K & 3) == 0 && (lda & 3) == 0 && ((uintptr_t)A & 15) == 0) {
        const int K4 = K >> 2;
        const long long n = (long long)rows * K4;
        for (long long i = threadIdx.x; i < n; i += 1024) {
            const int r = (int)(i / K4), c = (int)(i - (long long)r * K4);
            const float4 v = *reinterpret_cast<const float4*>(base + (size_t)r * lda + 4 * c);
            mn = fminf(mn, fminf(fminf(v.x, v.y), fminf(v.z, v.w)));
            mx = fmaxf(mx, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
        }
    } else {
        const long long n = (long long)rows * K;
        for (long long i = threadIdx.x; i < n; i += 1024) {
            const int r = (int)(i / K), c = (int)(i - (long long)r * K);
            const float v = base[(size_t)r * lda + c];
            mn = fminf(mn, v);
            mx = fmaxf(mx, v);
        }
    }
    __shared__ float smn[16], smx[16];
    mn = -wave_max(-mn);
    mx = wave_max(mx);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { smn[w] = mn; smx[w] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 16; ++i) { mn = fminf(mn, smn[i]); mx = fmaxf(mx, smx[i]); }
        // [UPSTREAM] onnxruntime GetQuantizationParameter: scale = max == min ? 1 : (max - min) / 255;
        // zero point = RoundHalfToEven(clamp(0 - min / scale, 0, 255))
        const float sx = mx == mn ? 1.0f : __fdiv_rn(mx - mn, 255.0f);
        const float zx = rintf(fminf(fmaxf(0.0f - __fdiv_rn(mn, sx), 0.0f), 255.0f));
        qp[2 * g] = sx;
        qp[2 * g + 1] = zx;
    }
}

struct GemmI8 {
    const float* A; const int8_t* W; const int32_t* colsum; const float* wq; const float* qp;
    float* out; const float* bias; const float* residual;
    int lda, ldw, ldc, M, N, K, group, flags;
};

// 256 threads = 4 waves over a 64 (activation rows) x 128 (weight rows) tile; wave w owns weight rows 32 w .. 32 w + 31 and all
// 64 activation rows: 2 x 4 MFMA tiles of 16 x 16.  The weight fragment is the MFMA's A operand (D rows = output columns n),
// the quantized activations its B operand (D columns = output rows m): D lane l holds n = 4 (l >> 4) + r, m = l & 15.  Both
// operands take byte j of lane l from k = 16 (l >> 4) + j of the tile; whatever k order the instruction uses inside a lane, it is
// the same for A and B, and an integer sum does not depend on the order.
__global__ __launch_bounds__(256) void gemm_i8q_kernel(GemmI8 p) {
    __shared__ __attribute__((aligned(16))) int8_t As[IBM * ILD];
    __shared__ __attribute__((aligned(16))) int8_t Ws[IBN * ILD];
    __shared__ int32_t rowsum_s[IBM];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int m0 = blockIdx.y * IBM, n0 = blockIdx.x * IBN;
    // A loader: row t / 4, 16 columns at (t % 4) * 16
    const int ar = t >> 2, aseg = (t & 3) * 16, am = m0 + ar;
    float sx = 1.0f, zx = 0.0f;
    if (am < p.M) {
        const int g = am / p.group;
        sx = p.qp[2 * g];
        zx = p.qp[2 * g + 1];
    }
    int rsum = 0;
    // W loader: row t / 2, 32 columns at (t % 2) * 32
    const int wr = t >> 1, wseg = (t & 1) * 32, wn = n0 + wr;
    const bool avec = (p.lda & 3) == 0 && ((uintptr_t)p.A & 15) == 0, wvec = (p.ldw & 15) == 0 && ((uintptr_t)p.W & 15) == 0;
    i32x4_t acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (i32x4_t){0, 0, 0, 0};
    for (int k0 = 0; k0 < p.K; k0 += IBK) {
        {
            float x[16];
            const int kb = k0 + aseg;
            int nv = 0;                                       // valid columns of this thread's 16
            if (am < p.M) {
                const float* src = p.A + (size_t)am * p.lda + kb;
                if (avec && kb + 16 <= p.K) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const float4 v = *reinterpret_cast<const float4*>(src + 4 * c);
                        x[4 * c] = v.x; x[4 * c + 1] = v.y; x[4 * c + 2] = v.z; x[4 * c + 3] = v.w;
                    }
                    nv = 16;
                } else {
                    nv = p.K - kb;
                    nv = nv < 0 ? 0 : (nv > 16 ? 16 : nv);
#pragma unroll
                    for (int e = 0; e < 16; ++e) x[e] = e < nv ? src[e] : 0.0f;
                }
            }
            int packed[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                unsigned u = 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int idx = 4 * c + e;
                    int a = 0;                                // padding columns: a = 0, no contribution whatever W holds there
                    if (idx < nv) a = (int)quant_u8(x[idx], sx, zx) - 128;
                    rsum += a;
                    u |= (unsigned)(a & 0xff) << (8 * e);
                }
                packed[c] = (int)u;
            }
            *reinterpret_cast<i32x4_t*>(As + ar * ILD + aseg) = (i32x4_t){packed[0], packed[1], packed[2], packed[3]};
        }
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int kb = k0 + wseg + 16 * c;
            i32x4_t v = {0, 0, 0, 0};
            if (wn < p.N) {
                const int8_t* src = p.W + (size_t)wn * p.ldw + kb;
                if (wvec && kb + 16 <= p.K) {
                    v = *reinterpret_cast<const i32x4_t*>(src);
                } else {
                    unsigned u[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                    for (int e = 0; e < 16; ++e)
                        if (kb + e < p.K) u[e >> 2] |= (unsigned)(uint8_t)src[e] << (8 * (e & 3));
                    v = (i32x4_t){(int)u[0], (int)u[1], (int)u[2], (int)u[3]};
                }
            }
            *reinterpret_cast<i32x4_t*>(Ws + wr * ILD + wseg + 16 * c) = v;
        }
        __syncthreads();
        const int fr = lane & 15, fk = 16 * (lane >> 4);
        i32x4_t wf[2], af[4];
#pragma unroll
        for (int i = 0; i < 2; ++i) wf[i] = *reinterpret_cast<const i32x4_t*>(Ws + (32 * w + 16 * i + fr) * ILD + fk);
#pragma unroll
        for (int j = 0; j < 4; ++j) af[j] = *reinterpret_cast<const i32x4_t*>(As + (16 * j + fr) * ILD + fk);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wf[i], af[j], acc[i][j], 0, 0, 0);
        __syncthreads();
    }
    // sum of a over the row's K columns: the four loader threads of a row are adjacent lanes
    rsum += __shfl_xor(rsum, 1, 64);
    rsum += __shfl_xor(rsum, 2, 64);
    if ((t & 3) == 0) rowsum_s[ar] = rsum;
    __syncthreads();
    const float sw = p.wq[0];
    const int zw = (int)p.wq[1];
    const bool has_bias = p.flags & RS_GEMM_BIAS, res = p.flags & RS_GEMM_RESIDUAL;
    const bool swl = p.flags & RS_GEMM_SWOOSHL, swr = p.flags & RS_GEMM_SWOOSHR;
    const bool ovec = (p.ldc & 3) == 0 && ((uintptr_t)p.out & 15) == 0 && (!res || ((uintptr_t)p.residual & 15) == 0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ml = 16 * j + (lane & 15), m = m0 + ml;
        if (m >= p.M) continue;
        const int g = m / p.group;
        const float gsx = p.qp[2 * g];
        const int zxi = (int)p.qp[2 * g + 1];
        const float scale = gsx * sw;                         // Mul(sx, sw)
        const int corr_row = zw * (rowsum_s[ml] + p.K * (128 - zxi));
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int nb = n0 + 32 * w + 16 * i + 4 * (lane >> 4);
            if (nb >= p.N) continue;
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = nb + r;
                if (n >= p.N) { v[r] = 0.0f; continue; }
                const int q = acc[i][j][r] + (128 - zxi) * p.colsum[n] - corr_row;
                float f = (float)q * scale;                   // Cast (round to nearest even), Mul
                if (has_bias) f = f + p.bias[n];
                if (swl) f = swoosh_l_exact(f);
                if (swr) f = swoosh_r_exact(f);
                if (res) f = f + p.residual[(size_t)m * p.ldc + n];
                v[r] = f;
            }
            float* dst = p.out + (size_t)m * p.ldc + nb;
            if (ovec && nb + 3 < p.N) {
                *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (nb + r < p.N) dst[r] = v[r];
            }
        }
    }
}

}  // namespace

int rs_launch_i8_range(rs_ctx* ctx, const float* A, int lda, const int32_t* lens, int group, int n_groups, int K, float* qp, hipStream_t s) {
    if (n_groups <= 0) return RS_OK;
    if (!A || !lens || !qp || group <= 0 || K <= 0 || lda < K) return rs_fail(ctx, RS_EINVAL, "i8 range: bad arguments (group %d, K %d, lda %d)", group, K, lda);
    hipLaunchKernelGGL(i8_range_kernel, dim3(n_groups), dim3(1024), 0, s, A, lda, lens, group, K, qp);
    RS_CHECK_LAUNCH(ctx, "i8 range");
    return RS_OK;
}

int rs_launch_gemm_i8q(rs_ctx* ctx, const float* A, int lda, int group, const float* qp, const int8_t* W, int ldw, const int32_t* colsum,
                       const float* wq, float* out, int ldc, int M, int N, int K, int flags, const float* bias, const float* residual, hipStream_t s) {
    if (M <= 0 || N <= 0) return RS_OK;
    if (K <= 0 || lda < K || ldw < K || ldc < N || group <= 0 || (ldw & 15) || ((uintptr_t)W & 15))
        return rs_fail(ctx, RS_EINVAL, "gemm_i8q: lda, ldw >= K, ldc >= N, ldw %% 16 and a 16-byte aligned weight required (M %d N %d K %d)", M, N, K);
    if (flags & ~(RS_GEMM_BIAS | RS_GEMM_RESIDUAL | RS_GEMM_OUT_F32 | RS_GEMM_SWOOSHL | RS_GEMM_SWOOSHR))
        return rs_fail(ctx, RS_EINVAL, "gemm_i8q: unsupported flags %d", flags);
    if ((flags & RS_GEMM_SWOOSHL) && (flags & RS_GEMM_SWOOSHR)) return rs_fail(ctx, RS_EINVAL, "gemm_i8q: SWOOSHL and SWOOSHR together");
    if ((flags & RS_GEMM_BIAS) && !bias) return rs_fail(ctx, RS_EINVAL, "gemm_i8q: bias flag without a bias");
    if ((flags & RS_GEMM_RESIDUAL) && !residual) return rs_fail(ctx, RS_EINVAL, "gemm_i8q: residual flag without a residual");
    if (!A || !W || !colsum || !wq || !qp || !out) return rs_fail(ctx, RS_EINVAL, "gemm_i8q: null pointer");
    GemmI8 p{A, W, colsum, wq, qp, out, bias, residual, lda, ldw, ldc, M, N, K, group, flags};
    const dim3 grid((N + IBN - 1) / IBN, (M + IBM - 1) / IBM), block(256);
    rs_prof_scope prof(ctx, RS_PROF_GEMM, s, 2.0 * M * (double)N * K, 4.0 * (double)M * K + (double)N * K + 4.0 * (double)M * N);
    hipLaunchKernelGGL(gemm_i8q_kernel, grid, block, 0, s, p);
    prof.end();
    RS_CHECK_LAUNCH(ctx, "gemm_i8q");
    return RS_OK;
}

extern "C" int rs_gemm_i8q(rs_ctx* ctx, const float* A, int lda, const int32_t* lens, int group, const int8_t* W, int ldw, const int32_t* colsum,
                           const float* wq, float* out, int ldc, int M, int N, int K, int flags, const float* bias, const float* residual, float* qp,
                           void* stream) {
    RS_GUARD(ctx, rs_gemm_i8q);
    if (M < 0 || N < 0) return rs_fail(ctx, RS_EINVAL, "gemm_i8q: negative size");
    if (M == 0 || N == 0) return RS_OK;
    if (group <= 0 || M % group) return rs_fail(ctx, RS_EINVAL, "gemm_i8q: M (%d) must be a whole number of groups of %d rows", M, group);
    const hipStream_t s = (hipStream_t)stream;
    if (int rc = rs_launch_i8_range(ctx, A, lda, lens, group, M / group, K, qp, s); rc != RS_OK) return rc;
    return rs_launch_gemm_i8q(ctx, A, lda, group, qp, W, ldw, colsum, wq, out, ldc, M, N, K, flags, bias, residual, s);
}
