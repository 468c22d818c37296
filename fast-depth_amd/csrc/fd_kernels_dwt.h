// fd_kernels_dwt.h -- depthwise TRANSPOSED k x k convolution (k = 3 or 5), stride 2, padding (k-1)/2, output padding 1, + folded BatchNorm + activation:
// the map-doubling unit of the reference's DeConv decoder (convt_dw, models.py:89-99), in polyphase form.
//
// out[2r+a][2c+b] = sum in[i][j] * w[2r+a-2i+p][2c+b-2j+p], p = (k-1)/2.  Written out by output parity (a, b) only the taps whose parity matches
// survive -- no product with an inserted zero is ever formed:
//     k = 5:  a = 0 -> i in {r-1, r, r+1}, ky in {4, 2, 0};   a = 1 -> i in {r, r+1}, ky in {3, 1}
//     k = 3:  a = 0 -> i = r, ky = 1;                          a = 1 -> i in {r, r+1}, ky in {2, 0}
// and the same table for the columns: the 2 x 2 output quad of input pixel (r, c) is a function of the 3 x 3 (k = 3: 2 x 2) input window around it,
// 9 + 6 + 6 + 4 = 25 (k = 3: 1 + 2 + 2 + 4 = 9) multiply-adds = k^2 / 4 per output.  Window pixels outside the map contribute nothing.
//
// Register-window form, as fd_dw3_rows: no LDS, no barrier.  Work-item q = x * (C / 4) + c4 owns four adjacent channels of input column x and walks
// down the input rows of its band with the three-row window (rows r-1, r, r+1; columns x-1, x, x+1) and its channels' k^2 folded fp32 taps in
// registers; every step loads the window's new bottom row (3 loads) and emits the two output rows 2r, 2r+1 of the window's centre row (4 stores).
// Consecutive lanes cover consecutive channels, then the next column: a wave's loads are contiguous and each of its stores covers runs of
// C elements (the b = 0 and b = 1 stores of a row together fill it).  4 channels = 16 bytes per lane in fp32 and 8 bytes in the 16-bit plans -- eight
// channels would need 200 registers for the 5x5 taps alone.  Arithmetic is fmaf in fp32 starting from the folded bias, in every plan.
// grid (ceil(W * C / 4 / 256), bands of TH input rows, images) through fd_xcd_image_map (the halo rows and the neighbour columns are re-read by other
// work-items of the same image: one XCD's L2); block 256.  Any H, W >= 1 (a 1 x 1 map has no neighbour inside); C % 4 == 0.
#pragma once
#include "fd_device.h"

__device__ __forceinline__ fd_f32x4 fd_dwt_fma4(fd_f32x4 v, fd_f32x4 w, fd_f32x4 a)
{
    fd_f32x4 r = {fmaf(v.x, w.x, a.x), fmaf(v.y, w.y, a.y), fmaf(v.z, w.z, a.z), fmaf(v.w, w.w, a.w)};
    return r;
}

// The folded bias t = beta - mean * gamma / sqrt(var + eps) of a transposed layer, evaluated in fp64 and rounded once.  fd_pack_fold's fp32 form
// is accurate to a few ulp of |mean * scale|, not of |t|: where beta and mean * scale cancel, its error is large against the layer's small
// outputs -- the element-wise bound of tests/deconv_ref.py is relative to |t|.  (The layers that existed before keep fd_pack_fold's bias: bit for bit.)
__global__ void __launch_bounds__(256)
fd_dwt_fold_bias(const float *__restrict__ gamma, const float *__restrict__ beta, const float *__restrict__ mean, const float *__restrict__ var,
                 float eps, float *__restrict__ bias, int cout)
{
    const int c = (int)(blockIdx.x * 256 + threadIdx.x);
    if (c < cout) bias[c] = (float)((double)beta[c] - (double)mean[c] * ((double)gamma[c] / sqrt((double)var[c] + (double)eps)));
}

template <typename T, int K, int ACT>
__global__ void __launch_bounds__(256)
fd_dwt_rows(const T *__restrict__ in, const float *__restrict__ wp, const float *__restrict__ bias, T *__restrict__ out, int H, int W, int C, int TH)
{
    static_assert(K == 3 || K == 5, "polyphase tables exist for k = 3 and k = 5");
    constexpr int P = (K - 1) / 2;
    typedef fd_lane<T, 4> LN;
    const int CG = C >> 2;
    const fd_blk3 blk = fd_xcd_image_map();
    const int q = blk.x * 256 + (int)threadIdx.x;
    if (q >= W * CG) return;
    const int x = q / CG, c4 = q - x * CG;
    const int n = blk.z;
    const int r0 = blk.y * TH;
    const int r1 = (r0 + TH < H) ? r0 + TH : H;
    fd_f32x4 w[K * K];
#pragma unroll
    for (int t = 0; t < K * K; ++t) w[t] = fd_ld4(wp + (long)t * C + c4 * 4);
    const fd_f32x4 b4 = fd_ld4(bias + c4 * 4);
    const T *img = in + (long)n * H * W * C + c4 * 4;
    const bool okl = x >= 1, okr = x + 1 < W;
    const int xl = okl ? x - 1 : x, xr = okr ? x + 1 : x;    // clamped: the loads are always issued inside the map, the padding is a select
    // window row: columns x-1, x, x+1 (k = 3 never reads the left column nor the row above)
    auto load_row = [&](int iy, fd_f32x4 (&v)[3]) {
        const bool oky = iy >= 0 && iy < H;
        const int qy = iy < 0 ? 0 : (iy >= H ? H - 1 : iy);
        const T *p = img + (long)qy * W * C;
        if (K == 5) { v[0] = LN::ld(p + (long)xl * C); if (!(oky && okl)) v[0] = fd_zero4(); }
        v[1] = LN::ld(p + (long)x * C); if (!oky) v[1] = fd_zero4();
        v[2] = LN::ld(p + (long)xr * C); if (!(oky && okr)) v[2] = fd_zero4();
    };
    const int Wo = 2 * W;
    T *o = out + (((long)n * 2 * H + 2 * r0) * Wo + 2 * x) * C + c4 * 4;
    fd_f32x4 win[3][3];
#pragma unroll
    for (int t = 0; t < 9; ++t) win[t / 3][t % 3] = fd_zero4();
    if (K == 5) load_row(r0 - 1, win[0]);
    load_row(r0, win[1]);
    for (int r = r0; r < r1; ++r) {
        load_row(r + 1, win[2]);
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                fd_f32x4 acc = b4;
#pragma unroll
                for (int ri = 0; ri < 3; ++ri) {
                    const int ky = a + P + 2 - 2 * ri;         // window row ri is input row r - 1 + ri
                    if (ky < 0 || ky >= K) continue;
#pragma unroll
                    for (int ci = 0; ci < 3; ++ci) {
                        const int kx = b + P + 2 - 2 * ci;
                        if (kx < 0 || kx >= K) continue;
                        acc = fd_dwt_fma4(win[ri][ci], w[ky * K + kx], acc);
                    }
                }
                LN::st(o + ((long)a * Wo + b) * C, fd_act4<ACT>(acc));
            }
        o += 2 * (long)Wo * C;
#pragma unroll
        for (int ci = 0; ci < 3; ++ci) { win[0][ci] = win[1][ci]; win[1][ci] = win[2][ci]; }
    }
}
