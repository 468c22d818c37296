// fd_kernels_conv.h -- dense k x k convolution (k = 3 or 5, stride 1, padding (k-1)/2) + folded BatchNorm + activation as an IMPLICIT GEMM on the
// matrix cores: the unit of the dense NNConv decoder (reference models.py:52-59, 246-251), FD_OP_CONV.
//
// In NHWC the A operand of output pixel (y, x) for ONE filter tap (ky, kx) is the contiguous run of cin channels of input pixel (y+ky-p, x+kx-p), so
// the layer is a sum over k^2 taps of pointwise GEMMs whose A rows are shifted:  M = B*H*W output pixels, N = cout, K = k^2 * cin with the reduction
// index running tap-major, channel-minor.  The skeleton is fd_pw_gemm_f32 / fd_pw_gemm_h16 (LDS-DMA 3-stage ring issued two K tiles ahead, counted
// vmcnt + raw s_barrier, 128-byte LDS rows with the XOR swizzle on the DMA source and on the fragment reads, XCD-aware 1-D grid); what is new is that
// every lane recomputes its A source address per K tile from (tap, channel offset):
//   * fp32:    v_mfma_f32_32x32x2_f32, BK = 32 channels of one tap per K tile
//   * 16-bit:  v_mfma_f32_32x32x16_{f16,bf16} (template parameter T = storage type), BK = 64, fp32 accumulators
//   * nearest x2 in front (upsample = 1): the A row of (y, x) is read from the half-size STORED map at (y>>1, x>>1); the upsampled tensor never exists
//   * a tap outside the (upsampled) map, and the channels of a ragged last K tile of a tap (cin % BK != 0), are read from a line of zeros that the
//     pack kernel writes behind the layer's packed weights -- LDS-DMA cannot select, and nothing is clamped to a neighbouring pixel.  The packed
//     weights are zero-padded per tap to the K tile as well, so padded K multiplies 0 by 0
//   * split K: with few M x N tiles (conv1: 1 568 rows, K = 25 600 at batch 32) the K tiles are dealt to gridDim.y workgroups per output tile; each
//     writes its fp32 partial tile (split 0 starts at the bias) and fd_conv_reduce adds the partials IN SPLIT ORDER, activates and stores.  No
//     floating-point atomics: the same plan on the same input gives the same bits
// The taps are NOT pre-summed per output parity class (the polyphase form of a conv behind a nearest x2): every layer does its full k^2 * cin reduction.
// Ragged M / N: source rows are clamped (rows of A only reach the same rows of D, which are never stored); stores are guarded.
#pragma once
#include <type_traits>
#include "fd_kernels_h16.h"

#define FD_CONV_STAGES 3
#define FD_CONV_ROW_BYTES 128       // one LDS row = one K tile of one A / weight row
// elements of the reduction per K tile for an element size: 32 (fp32) / 64 (16-bit).  The ONE definition that the kernel, the packed layout (fd_conv_pack,
// fd_plan_pack_weights) and the plan's tiling (plan_layers) share
constexpr int fd_conv_bk(size_t esz) { return (int)(FD_CONV_ROW_BYTES / esz); }
#define FD_CONV_ZERO_BYTES 256      // the zero line behind a layer's packed weights (a K tile row is 128 bytes)

struct fd_conv_geo {
    int H, W;                // output map == logical (upsampled) input map
    int up;                  // 1: the stored input map is (H/2) x (W/2), read at (y>>1, x>>1)
    int ks;                  // 3 or 5
    int cin, cout;
    int ktpt;                // K tiles per tap = ceil(cin / BK); the packed weight rows hold ks*ks*ktpt*BK elements
    int m_tiles, n_tiles;
    int tps;                 // K tiles per split (gridDim.y splits)
    int act;                 // FD_ACT_*_ applied by the kernel that stores the output
};

__device__ __forceinline__ float fd_conv_act(float v, int act)
{
    return act == FD_ACT_RELU_ ? fd_act<FD_ACT_RELU_>(v) : (act == FD_ACT_RELU6_ ? fd_act<FD_ACT_RELU6_>(v) : v);
}

// ------------------------------------------------------------------------------------------------
// Weight packing: torch's [cout][cin][ky][kx] -> wp[cout][tap][cpad] (cpad = cin rounded up to the K tile, zero-padded), folded with the BatchNorm
// scale in fp64 and rounded to fp32 (16-bit plans: then once more to the storage type); then the zero line.  The bias is folded by fd_dwt_fold_bias (fp64, rounded once).
// ------------------------------------------------------------------------------------------------
template <typename TW>
__global__ void __launch_bounds__(256)
fd_conv_pack(const float *__restrict__ w, const float *__restrict__ gamma, const float *__restrict__ var, float eps,
             TW *__restrict__ wp, int cout, int cin, int kk, int cpad, long upto)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const long per = (long)kk * cpad, total = (long)cout * per;
    if (idx < total) {
        const int co = (int)(idx / per);
        const int rem = (int)(idx - (long)co * per);
        const int tap = rem / cpad, c = rem - tap * cpad;
        float v = 0.0f;
        if (c < cin) {
            const double scale = (double)gamma[co] / sqrt((double)var[co] + (double)eps);
            v = (float)((double)w[((long)co * cin + c) * kk + tap] * scale);
        }
        fd_st1(wp + idx, v);
    } else if (idx < upto) {                               // the zero line (upto = the layer's packed bytes / sizeof(TW))
        fd_st1(wp + idx, 0.0f);
    }
}

// ------------------------------------------------------------------------------------------------
// The implicit GEMM.  4 waves as WGM x WGN, each wave owns TM x TN accumulator tiles of 32 x 32.
// in: stored input [B][H>>up][W>>up][cin]; wp / zero: fd_conv_pack's output; part: fp32 partial tiles [splits][M][cout] (gridDim.y > 1 only).
// ------------------------------------------------------------------------------------------------
template <typename T, int WGM, int WGN, int TM, int TN>
__global__ void __launch_bounds__(256)
fd_conv_gemm(const T *__restrict__ in, const T *__restrict__ wp, const T *__restrict__ zero, const float *__restrict__ bias,
             T *__restrict__ out, float *__restrict__ part, int M, const fd_conv_geo g)
{
    static_assert(WGM * WGN == 4, "four waves per workgroup");
    constexpr bool F32 = std::is_same<T, float>::value;
    constexpr int BM = WGM * TM * 32, BN = WGN * TN * 32;
    constexpr int BK = fd_conv_bk(sizeof(T));               // elements per 128-byte LDS row
    constexpr int CH = 16 / (int)sizeof(T);                 // elements per 16-byte chunk
    constexpr int STAGE = (BM + BN) * 128;                  // bytes per stage
    constexpr int AG = BM / 32, RG = (BM + BN) / 32;        // LDS-DMA instructions (8 rows = 1 KiB each) per wave per K tile: AG of A rows, then the weight rows
    FD_DYN_SMEM(smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WGN, wn = wave - wm * WGN;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int nt = slot % g.n_tiles, mt = (slot / g.n_tiles) * 8 + xcd;
    if (mt >= g.m_tiles) return;
    const long m0 = (long)mt * BM;
    const int n0 = nt * BN;
    const int N = g.cout, kk = g.ks * g.ks, pad = g.ks >> 1;
    const int Hs = g.H >> g.up, Ws = g.W >> g.up;
    const int t0 = (int)blockIdx.y * g.tps;
    const int t1 = t0 + g.tps < kk * g.ktpt ? t0 + g.tps : kk * g.ktpt;

    // ---- LDS-DMA sources: this lane's row / swizzled chunk for each of the wave's row groups ----
    int src_k[RG];                                           // element offset of the chunk that lands in LDS slot (r, lane & 7)
    int ay[AG], ax[AG];                                      // A rows: the output pixel's coordinates ...
    long apix[AG];                                           // ... and the first stored pixel of its image
    const T *bsrc[RG - AG];                                  // weight rows
#pragma unroll
    for (int i = 0; i < RG; ++i) {
        const int r = (wave + 4 * i) * 8 + (lane >> 3);
        src_k[i] = ((lane & 7) ^ ((r >> 1) & 7)) * CH;
        if (i < AG) {
            long m = m0 + r;
            if (m > M - 1) m = M - 1;
            const long n = m / ((long)g.H * g.W);
            const int rem = (int)(m - n * g.H * g.W);
            ay[i] = rem / g.W; ax[i] = rem - ay[i] * g.W;
            apix[i] = n * Hs * Ws;
        } else {
            int row = n0 + (r - BM);
            if (row > N - 1) row = N - 1;
            bsrc[i - AG] = wp + (long)row * kk * g.ktpt * BK + src_k[i];
        }
    }
    auto issue = [&](int t) {
        const int tap = t / g.ktpt, kc = (t - tap * g.ktpt) * BK;
        const int ky = tap / g.ks, kx = tap - ky * g.ks;
        unsigned char *dst = smem + ((t - t0) % FD_CONV_STAGES) * STAGE + wave * 8 * 128;
#pragma unroll
        for (int i = 0; i < RG; ++i) {
            const T *s;
            if (i < AG) {
                const int iy = ay[i < AG ? i : 0] + ky - pad, ix = ax[i < AG ? i : 0] + kx - pad;
                const bool ok = (unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W && kc + src_k[i] < g.cin;
                s = ok ? in + ((apix[i < AG ? i : 0] + (long)(iy >> g.up) * Ws + (ix >> g.up)) * g.cin + kc + src_k[i]) : zero + src_k[i];
            } else {
                s = bsrc[i >= AG ? i - AG : 0] + (long)t * BK;
            }
            fd_glds16(reinterpret_cast<const float *>(s), reinterpret_cast<float *>(dst + i * 4 * 8 * 128));
        }
    };

    // accumulators: the folded-BN bias of their column in split 0, zero in the others
    fd_f32x16 acc[TM][TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int col = n0 + (wn * TN + j) * 32 + (lane & 31);
        const float bv = (col < N && blockIdx.y == 0) ? bias[col] : 0.0f;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = bv;
    }

    // ---- fragment read offsets (bytes) within a stage: row*128 + ((2s + h) ^ swz(row))*16 ----
    const int h = lane >> 5;
    int a_off[TM][4], b_off[TN][4];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int row = (wm * TM + i) * 32 + (lane & 31);
#pragma unroll
        for (int s = 0; s < 4; ++s) a_off[i][s] = row * 128 + (((2 * s + h) ^ ((row >> 1) & 7)) << 4);
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int row = BM + (wn * TN + j) * 32 + (lane & 31);
#pragma unroll
        for (int s = 0; s < 4; ++s) b_off[j][s] = row * 128 + (((2 * s + h) ^ ((row >> 1) & 7)) << 4);
    }

    issue(t0);
    if (t0 + 1 < t1) issue(t0 + 1);
    for (int t = t0; t < t1; ++t) {
        if (t + 1 < t1) fd_wait_vmcnt<RG>(); else fd_wait_vmcnt<0>();     // leave only tile t+1's loads in flight
        fd_block_barrier();                                  // tile t landed for every wave; the stage of tile t+2 is free again
        if (t + FD_CONV_STAGES - 1 < t1) issue(t + FD_CONV_STAGES - 1);
        const unsigned char *cur = smem + ((t - t0) % FD_CONV_STAGES) * STAGE;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            if constexpr (F32) {
                // a lane's 16-byte chunk is 4 consecutive k of its row (lanes 0-31 chunk 2s, lanes 32-63 chunk 2s+1): four MFMA steps
                fd_f32x4 a[TM], b[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i) a[i] = *reinterpret_cast<const fd_f32x4 *>(cur + a_off[i][s]);
#pragma unroll
                for (int j = 0; j < TN; ++j) b[j] = *reinterpret_cast<const fd_f32x4 *>(cur + b_off[j][s]);
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][q], b[j][q], acc[i][j], 0, 0, 0);
            } else {
                // a lane's 16-byte chunk IS the MFMA operand: 8 consecutive k of its row
                fd_u16x8 a[TM], b[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i) a[i] = *reinterpret_cast<const fd_u16x8 *>(cur + a_off[i][s]);
#pragma unroll
                for (int j = 0; j < TN; ++j) b[j] = *reinterpret_cast<const fd_u16x8 *>(cur + b_off[j][s]);
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = fd_mfma_32x32x16(T{}, a[i], b[j], acc[i][j]);
            }
        }
    }

    // epilogue: D register r of lane l is row (r&3) + 8*(r>>2) + 4*(l>>5), column l&31 of the 32x32 tile
    const bool split = gridDim.y > 1;
    float *pbase = split ? part + (long)blockIdx.y * M * N : nullptr;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int col = n0 + (wn * TN + j) * 32 + (lane & 31);
        if (col >= N) continue;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const long rbase = m0 + (wm * TM + i) * 32 + 4 * (lane >> 5);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long row = rbase + (r & 3) + 8 * (r >> 2);
                if (row >= M) continue;
                if (split) pbase[row * N + col] = acc[i][j][r];
                else fd_st1(out + row * N + col, fd_conv_act(acc[i][j][r], g.act));
            }
        }
    }
}

// the split-K epilogue: out = act(part[0] + part[1] + ... ) in split order, 4 consecutive channels per work-item (total = M * cout, a multiple of 4)
template <typename T>
__global__ void __launch_bounds__(256)
fd_conv_reduce(const float *__restrict__ part, T *__restrict__ out, long total, int splits, int act)
{
    const long e = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (e >= total) return;
    fd_f32x4 v = fd_ld4(part + e);
    for (int s = 1; s < splits; ++s) v += fd_ld4(part + (long)s * total + e);
    v.x = fd_conv_act(v.x, act); v.y = fd_conv_act(v.y, act); v.z = fd_conv_act(v.z, act); v.w = fd_conv_act(v.w, act);
    fd_st4(out + e, v);
}
