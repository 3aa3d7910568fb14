// Float32 arithmetic mode of the MLP engine (CS_FLAG_FP32): the per-layer path of run_forward / run_backward on float32
// operands and activations, contracted on gfx950's f32-input MFMA (v_mfma_f32_32x32x2_f32: exact float32 products, one
// rounding per fused multiply-add, 1/16 of the bf16 rate).  No bf16 instruction and no bf16 buffer anywhere on this path.
//
//   k_prepare_input_f32   : gather + normalise (k_prepare_input's arithmetic) into a float32 [m_pad][Kp] H0
//   k_gemm_f32<EPI, WT>   : out[m][j] = sum_k A[m][k] * B(k, j), A = activations / dz (k contiguous), B read straight from the
//                           float32 master weights P ([K][N], internal order): B(k, j) = W[k][j] (forward, WT = false) or
//                           W[j][k] (data gradient, WT = true); rows of W at or past `w_rows` read as zero (K need not be a
//                           multiple of 4: 425, 557).  Epilogues EPI_HIDDEN / EPI_OUT / EPI_DGRAD as k_gemm_nt's.
//   k_wgrad_f32           : dW = H^T dZ, db = column sums of dZ for ALL layers in one launch, row-split; split 0 stores into
//                           the gradient buffer, split s > 0 into partial-sum buffer s - 1 that the optimiser adds (OptArgs.Gx):
//                           no atomics, a fixed summation order - two runs on the same data give the same bits.
//
// Tiles: BM x BN outputs per 256-thread workgroup (128 x 128 or 64 x 64), 2 x 2 waves, 32-deep k slabs double-buffered in LDS
// with the next slab's global loads in flight during the current slab's MFMAs.  LDS holds both operands k-major ([k][i],
// [k][j]): a lane's MFMA operand is one ds_read_b32, the 32 lanes of a half-wave read 32 consecutive floats.
#pragma once
#include "kernels.h"

#define F32_BK 32                // contraction slab
#define F32_PAD 4                // LDS row pad (floats): keeps 16-B alignment, breaks the power-of-two row pitch
#define CS_WGRAD_F32_PARTS 7     // partial-sum buffers of a float32 handle (training steps with <= 8 row splits)

struct GemmF32 {
    const float* A; int lda;     // [m_pad][lda] activations / dz, contraction index contiguous
    const float* W; int ldw;     // float32 master weights of the layer, [w_rows][ldw] (P + w_off)
    int w_rows;                  // rows of W that exist (K of the layer); rows past it read as zero
    int K;                       // contraction length (real; slabs past it see zero weights)
    int N;                       // output width, multiple of the tile
    int act; float alpha;
    // EPI_HIDDEN / EPI_OUT
    const float* bias;           // [N]
    float* out; int ldo;         // float32 output [m_pad][ldo] (hidden activation, dz of the heads / of the previous layer)
    // EPI_OUT (as GemmNT)
    int n_lin, n_real;
    float* yhat; const float* y; const int64_t* row_idx; int64_t n_rows;
    float* loss; int loss_stripes; int loss_kind; const float* keep;
    // EPI_DGRAD
    const float* hprev; int ldh;  // activation output of the previous layer (same shape as out)
};

// gather + normalise as k_prepare_input (prepare4), float32 out; pad rows and columns are zero.
__global__ __launch_bounds__(256) void k_prepare_input_f32(const float* __restrict__ x, const int64_t* __restrict__ row_idx,
                                                           int64_t n, int64_t m_pad, int n_in, int kp,
                                                           const float* __restrict__ sub, const float* __restrict__ div,
                                                           int normalise, float* __restrict__ h0) {
    const int groups = kp >> 2;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= m_pad * groups) return;
    const int64_t m = gid / groups;
    const int c = (int)(gid - m * groups) * 4;
    float v[4];
    prepare4(x, row_idx, n, n_in, sub, div, normalise, m, c, v);
    *reinterpret_cast<float4*>(h0 + m * kp + c) = make_float4(v[0], v[1], v[2], v[3]);
}

// One 32-deep slab of a BM x BN tile: lane (r = l & 31, h = l >> 5) feeds k = 2 kk + h of every MFMA; the W side is the MFMA's
// A operand (result rows = output columns j), the activation side its B operand (result columns = output rows i), so a lane ends
// up owning 4 consecutive j of one row i (registers 4q..4q+3: j = 8q + 4h + 0..3) - float4 epilogue stores.
template <int TM, int TN>
__device__ __forceinline__ void f32_slab(const float* __restrict__ xs, int ldx, const float* __restrict__ ws, int ldwl, int xi0,
                                         int wj0, int lane, f32x16_t (&acc)[TN][TM]) {
    const int r = lane & 31, h = lane >> 5;
#pragma unroll
    for (int kk = 0; kk < F32_BK / 2; ++kk) {
        const int k = 2 * kk + h;
        float xa[TM], wb[TN];
#pragma unroll
        for (int t = 0; t < TM; ++t) xa[t] = xs[k * ldx + xi0 + t * 32 + r];
#pragma unroll
        for (int t = 0; t < TN; ++t) wb[t] = ws[k * ldwl + wj0 + t * 32 + r];
#pragma unroll
        for (int tj = 0; tj < TN; ++tj)
#pragma unroll
            for (int ti = 0; ti < TM; ++ti) acc[tj][ti] = __builtin_amdgcn_mfma_f32_32x32x2f32(wb[tj], xa[ti], acc[tj][ti], 0, 0, 0);
    }
}

template <int EPI, bool WT, int BM, int BN>
__global__ __launch_bounds__(256) void k_gemm_f32(const GemmF32 p) {
    constexpr int LX = BM + F32_PAD, LW = BN + F32_PAD;
    constexpr int TM = BM / 64, TN = BN / 64;          // 32 x 32 MFMA tiles per wave and dimension
    constexpr int NA = BM / 32, NB = BN / 32;          // float4 loads per thread and slab
    __shared__ __attribute__((aligned(16))) float xs[2][F32_BK * LX];
    __shared__ __attribute__((aligned(16))) float wsm[2][F32_BK * LW];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid >> 1, wn = wid & 1;
    const int64_t m0 = (int64_t)blockIdx.x * BM;
    const int j0 = blockIdx.y * BN;
    float4 ra[NA], rb[NB];
    // A: chunk c -> row c / 8, k quad c % 8 (8 lanes read one 128-B row piece)
    auto gload = [&](int k0) {
#pragma unroll
        for (int q = 0; q < NA; ++q) {
            const int c = tid + 256 * q, i = c >> 3, kq = c & 7;
            ra[q] = *reinterpret_cast<const float4*>(p.A + (m0 + i) * p.lda + k0 + 4 * kq);
        }
#pragma unroll
        for (int q = 0; q < NB; ++q) {
            const int c = tid + 256 * q;
            if (!WT) {                                 // W[k][j]: row k0 + c / (BN/4), 4 consecutive j
                const int kr = c / (BN / 4), jq = c % (BN / 4);
                const int k = k0 + kr;
                rb[q] = k < p.w_rows ? *reinterpret_cast<const float4*>(p.W + (int64_t)k * p.ldw + j0 + 4 * jq) : make_float4(0.f, 0.f, 0.f, 0.f);
            } else {                                   // W[j][k]: row j0 + c / 8, 4 consecutive k
                const int j = j0 + (c >> 3), kq = c & 7;
                rb[q] = j < p.w_rows ? *reinterpret_cast<const float4*>(p.W + (int64_t)j * p.ldw + k0 + 4 * kq) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    };
    auto sstore = [&](int buf) {
#pragma unroll
        for (int q = 0; q < NA; ++q) {
            const int c = tid + 256 * q, i = c >> 3, kq = c & 7;
            float* d = xs[buf] + (4 * kq) * LX + i;
            d[0] = ra[q].x; d[LX] = ra[q].y; d[2 * LX] = ra[q].z; d[3 * LX] = ra[q].w;
        }
#pragma unroll
        for (int q = 0; q < NB; ++q) {
            const int c = tid + 256 * q;
            if (!WT) {
                const int kr = c / (BN / 4), jq = c % (BN / 4);
                *reinterpret_cast<float4*>(wsm[buf] + kr * LW + 4 * jq) = rb[q];
            } else {
                const int j = c >> 3, kq = c & 7;
                float* d = wsm[buf] + (4 * kq) * LW + j;
                d[0] = rb[q].x; d[LW] = rb[q].y; d[2 * LW] = rb[q].z; d[3 * LW] = rb[q].w;
            }
        }
    };
    f32x16_t acc[TN][TM];
#pragma unroll
    for (int a = 0; a < TN; ++a)
#pragma unroll
        for (int b = 0; b < TM; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    const int nt = (p.K + F32_BK - 1) / F32_BK;
    gload(0);
    sstore(0);
    __syncthreads();
    for (int t = 0; t < nt; ++t) {
        if (t + 1 < nt) gload((t + 1) * F32_BK);
        f32_slab<TM, TN>(xs[t & 1], LX, wsm[t & 1], LW, wm * (BM / 2), wn * (BN / 2), lane, acc);
        if (t + 1 < nt) sstore((t + 1) & 1);
        __syncthreads();
    }

    // ---- epilogue: lane owns row m = .. + (lane & 31), columns n = .. + 8q + 4 (lane >> 5) + 0..3
    float sq = 0.f, ab = 0.f;
#pragma unroll
    for (int tj = 0; tj < TN; ++tj) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int n = j0 + wn * (BN / 2) + tj * 32 + 8 * q + 4 * (lane >> 5);
            float4 b4 = make_float4(0.f, 0.f, 0.f, 0.f);
            if (EPI != EPI_DGRAD) b4 = *reinterpret_cast<const float4*>(p.bias + n);
#pragma unroll
            for (int ti = 0; ti < TM; ++ti) {
                const int64_t m = m0 + wm * (BM / 2) + ti * 32 + (lane & 31);
                float v[4] = {acc[tj][ti][4 * q + 0], acc[tj][ti][4 * q + 1], acc[tj][ti][4 * q + 2], acc[tj][ti][4 * q + 3]};
                if (EPI == EPI_HIDDEN) {
                    v[0] = act_fwd(v[0] + b4.x, p.act, p.alpha); v[1] = act_fwd(v[1] + b4.y, p.act, p.alpha);
                    v[2] = act_fwd(v[2] + b4.z, p.act, p.alpha); v[3] = act_fwd(v[3] + b4.w, p.act, p.alpha);
                    *reinterpret_cast<float4*>(p.out + m * p.ldo + n) = make_float4(v[0], v[1], v[2], v[3]);
                } else if (EPI == EPI_DGRAD) {
                    const float4 hh = *reinterpret_cast<const float4*>(p.hprev + m * p.ldh + n);
                    v[0] *= act_bwd_from_h(hh.x, p.act, p.alpha); v[1] *= act_bwd_from_h(hh.y, p.act, p.alpha);
                    v[2] *= act_bwd_from_h(hh.z, p.act, p.alpha); v[3] *= act_bwd_from_h(hh.w, p.act, p.alpha);
                    *reinterpret_cast<float4*>(p.out + m * p.ldo + n) = make_float4(v[0], v[1], v[2], v[3]);
                } else {  // EPI_OUT
                    v[0] += b4.x; v[1] += b4.y; v[2] += b4.z; v[3] += b4.w;
                    float d[4];
                    const bool valid = m < p.n_rows && n < p.n_real;
                    float4 t4 = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (p.y && valid) t4 = *reinterpret_cast<const float4*>(p.y + (p.row_idx ? p.row_idx[m] : m) * p.n_real + n);
                    head4(v, d, n >= p.n_lin, p.keep, n, p.y && valid, t4, p.loss_kind, sq, ab);   // (n_lin is a multiple of 4)
                    if (valid && p.yhat)
                        *reinterpret_cast<float4*>(p.yhat + m * p.n_real + n) = make_float4(v[0], v[1], v[2], v[3]);
                    if (p.out) *reinterpret_cast<float4*>(p.out + m * p.ldo + n) = make_float4(d[0], d[1], d[2], d[3]);
                }
            }
        }
    }
    if (EPI == EPI_OUT && p.y) {
        __shared__ float red[8];
        loss_flush(p.loss, p.loss_stripes, blockIdx.x + blockIdx.y, sq, ab, red, tid, 4);
    }
}

// ---------------------------------------------------------------- weight gradients
struct WgradF32Layer {
    const float* H; int ldh;     // [m_pad][ldh] layer input activations
    const float* Z; int ldz;     // [m_pad][ldz] dz of the layer
    float* dW; int N;            // [K][N] in the gradient buffer
    int k_real;                  // rows of dW that exist
    float* db;                   // [N]
    int tiles_i, tiles_j;        // output tiles over (Kp, N)
    int wg_begin;                // first workgroup of this layer in the grouped grid
};
struct WgradF32Args {
    int n_layers;
    WgradF32Layer L[WGRAD_MAX_LAYERS];
    int64_t m_pad;               // multiple of 128; rows >= n hold zeros in Z
    int splitk;                  // row-range splits per tile (same for every layer)
    int accumulate;              // 1: dW += (one split only: cs_mlp_loss_grads); 0: split 0 stores, split s > 0 stores into part s - 1
    const float* g_base; float* part; int64_t part_stride;
};

template <int BT>
__global__ __launch_bounds__(256) void k_wgrad_f32(const WgradF32Args pa) {
    constexpr int LD = BT + F32_PAD, T = BT / 64, NQ = BT / 32;      // NQ: float4 loads per operand, thread and slab (2 or 4)
    __shared__ __attribute__((aligned(16))) float hs[2][F32_BK * LD];
    __shared__ __attribute__((aligned(16))) float zs[2][F32_BK * LD];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid >> 1, wn = wid & 1;
    const int b = (int)blockIdx.x;
    int l = 0;
    while (l + 1 < pa.n_layers && b >= pa.L[l + 1].wg_begin) ++l;
    const WgradF32Layer& ly = pa.L[l];
    const int per_split = ly.tiles_i * ly.tiles_j;
    int rel = b - ly.wg_begin;
    const int split = rel / per_split;
    rel -= split * per_split;
    const int ti = rel / ly.tiles_j, tj = rel - ti * ly.tiles_j;
    const int i0 = ti * BT, j0 = tj * BT;
    const int slabs = (int)(pa.m_pad / F32_BK);
    const int s0 = (int)((int64_t)slabs * split / pa.splitk), s1 = (int)((int64_t)slabs * (split + 1) / pa.splitk);
    const bool do_db = ti == 0;
    // chunk c = tid + 256 q -> slab row c / (BT/4), 4 consecutive columns: both operands are read row by row, no transposition
    const int rr0 = tid / (BT / 4), cq = tid % (BT / 4), rstep = 256 / (BT / 4);
    const float* hg = ly.H + (int64_t)rr0 * ly.ldh + i0 + 4 * cq;
    const float* zg = ly.Z + (int64_t)rr0 * ly.ldz + j0 + 4 * cq;
    // named scalars, not arrays: arrays indexed in these loops were left in scratch memory (see k_gemm_nt)
    float4 rh0, rh1, rh2, rh3, rz0, rz1, rz2, rz3;
#define WF_GLOAD(s)                                                                                       \
    {                                                                                                     \
        const int64_t r_ = (int64_t)(s) * F32_BK;                                                         \
        rh0 = *reinterpret_cast<const float4*>(hg + (r_ + 0 * rstep) * ly.ldh);                           \
        rz0 = *reinterpret_cast<const float4*>(zg + (r_ + 0 * rstep) * ly.ldz);                           \
        rh1 = *reinterpret_cast<const float4*>(hg + (r_ + 1 * rstep) * ly.ldh);                           \
        rz1 = *reinterpret_cast<const float4*>(zg + (r_ + 1 * rstep) * ly.ldz);                           \
        if (NQ > 2) {                                                                                     \
            rh2 = *reinterpret_cast<const float4*>(hg + (r_ + 2 * rstep) * ly.ldh);                       \
            rz2 = *reinterpret_cast<const float4*>(zg + (r_ + 2 * rstep) * ly.ldz);                       \
            rh3 = *reinterpret_cast<const float4*>(hg + (r_ + 3 * rstep) * ly.ldh);                       \
            rz3 = *reinterpret_cast<const float4*>(zg + (r_ + 3 * rstep) * ly.ldz);                       \
        }                                                                                                 \
    }
#define WF_SSTORE(buf)                                                                                    \
    {                                                                                                     \
        float* h_ = hs[buf] + rr0 * LD + 4 * cq;                                                          \
        float* z_ = zs[buf] + rr0 * LD + 4 * cq;                                                          \
        *reinterpret_cast<float4*>(h_) = rh0; *reinterpret_cast<float4*>(z_) = rz0;                       \
        *reinterpret_cast<float4*>(h_ + rstep * LD) = rh1; *reinterpret_cast<float4*>(z_ + rstep * LD) = rz1; \
        if (NQ > 2) {                                                                                     \
            *reinterpret_cast<float4*>(h_ + 2 * rstep * LD) = rh2; *reinterpret_cast<float4*>(z_ + 2 * rstep * LD) = rz2; \
            *reinterpret_cast<float4*>(h_ + 3 * rstep * LD) = rh3; *reinterpret_cast<float4*>(z_ + 3 * rstep * LD) = rz3; \
        }                                                                                                 \
    }
    f32x16_t acc[T][T];
#pragma unroll
    for (int a = 0; a < T; ++a)
#pragma unroll
        for (int c = 0; c < T; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][c][r] = 0.f;
    float colsum = 0.f;                                // db: thread tid < BT sums column j0 + tid of dZ, rows in order
    WF_GLOAD(s0)                                       // (the host keeps splitk <= slabs: every split has a slab)
    WF_SSTORE(0)
    __syncthreads();
    for (int s = s0; s < s1; ++s) {
        const int buf = (s - s0) & 1;
        if (s + 1 < s1) { WF_GLOAD(s + 1) }
        f32_slab<T, T>(hs[buf], LD, zs[buf], LD, wm * (BT / 2), wn * (BT / 2), lane, acc);
        if (do_db && tid < BT) {
#pragma unroll 8
            for (int r = 0; r < F32_BK; ++r) colsum += zs[buf][r * LD + tid];
        }
        if (s + 1 < s1) { WF_SSTORE(buf ^ 1) }
        __syncthreads();
    }
#undef WF_GLOAD
#undef WF_SSTORE
    // destination: the gradient buffer (split 0) or partial-sum buffer split - 1 at the same offset
    float* dW = ly.dW;
    float* db = ly.db;
    if (split > 0) {
        const int64_t shift = (int64_t)(split - 1) * pa.part_stride + (pa.part - pa.g_base);
        dW += shift; db += shift;
    }
#pragma unroll
    for (int a = 0; a < T; ++a) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int n = j0 + wn * (BT / 2) + a * 32 + 8 * q + 4 * (lane >> 5);
#pragma unroll
            for (int c = 0; c < T; ++c) {
                const int k = i0 + wm * (BT / 2) + c * 32 + (lane & 31);
                if (k >= ly.k_real) continue;
                float4 v = make_float4(acc[a][c][4 * q + 0], acc[a][c][4 * q + 1], acc[a][c][4 * q + 2], acc[a][c][4 * q + 3]);
                float4* d = reinterpret_cast<float4*>(dW + (int64_t)k * ly.N + n);
                if (pa.accumulate) { const float4 o = *d; v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w; }
                *d = v;
            }
        }
    }
    if (do_db && tid < BT) {
        float* d = db + j0 + tid;
        *d = pa.accumulate ? *d + colsum : colsum;
    }
}
