// fd_kernels_dwb.h -- the two primitives of the reference's bilinear decoder BLConv(k, dw=True) (models.py:272-294):
//
//   fd_dwb_rows<T, K, ACT>     depthwise k x k convolution (k = 3 or 5, stride 1, padding (k-1)/2) + folded BatchNorm + activation ON THE BILINEAR x2
//                              (F.interpolate(scale_factor=2, mode='bilinear', align_corners=False)) of its producer's stored output: the upsampled
//                              tensor is never written, the kernel interpolates in registers
//   fd_head_bilinear<T, ACT>   the last layer, pointwise Cin -> 1 + folded BatchNorm, evaluated on the HALF-SIZE map, then interpolated, activated and
//                              written as the fp32 NCHW network output
//
// Interpolation.  Bilinear x2 with align_corners=False is separable, with weights 1/4 and 3/4 and a CLAMPED source index:
//     up[2y]   = 1/4 s[max(y-1, 0)] + 3/4 s[y]          up[2y+1] = 3/4 s[y] + 1/4 s[min(y+1, h-1)]
// and the same rule for the columns.  Written for up row 2y + U with m = floor(U / 2): U even -> 1/4 s[y+m-1] + 3/4 s[y+m], U odd ->
// 3/4 s[y+m] + 1/4 s[y+m+1].  One step is fmaf(0.75, major, 0.25 * minor): the product with 1/4 is exact, so a step rounds once.
//
// Two border rules meet in fd_dwb_rows.  (1) Up-pixels INSIDE [0, 2h) x [0, 2w) at the border use the clamped (replicated) source: every load is issued
// at an index clamped into the map and its value is USED.  (2) The k x k convolution zero-pads the UPSAMPLED map: up-pixels outside it are zero.  That is
// a select (columns: on the horizontally interpolated value; rows: the up-row's whole contribution is passed over, a workgroup-uniform branch), never a
// product with zero, so a non-finite value next to the border does not leak into a pixel that must not see it.
//
// fd_dwb_rows is the register-window, row-walking form of fd_dwt_rows / fd_dws_rows: no LDS, no barrier.  Work-item q = x * (C / 2) + cg owns source
// column x and 2 adjacent channels; consecutive lanes take consecutive channel pairs, then the next column, so a wave's loads and stores are contiguous.
// With p = (k-1)/2 the 2 x 2 output quad of source pixel (y, x) reads up rows 2y-p .. 2y+p+1 (k+1 of them), which come from source rows y-R .. y+R,
// R = p (k = 5: the 5 x 5 window, k = 3: the 3 x 3 window); columns alike.  A source row is interpolated HORIZONTALLY ON LOAD: 2R+1 loads become the k+1
// up-columns the lane needs, kept in fp32 registers -- the window is (2R+1) rows x (k+1) columns x 2 channels (k = 5: 60 registers, k = 3: 24).  A step
// loads the window's new bottom row, then for each of the k+1 up rows forms it by the vertical step and adds its products into the (at most two) output
// rows that meet it: out(2y+a, 2x+b) += up[a+ky][b+kx] * w[ky][kx].  Plain fp32 fmaf / multiply only; every accumulator starts from the folded bias.
// Two channels per lane: with four, the k = 5 window (120) and taps (100) alone exceed 200 registers.
// Taps: fd_pack_fold's tap-major fp32 [k^2][C]; bias: fd_dwt_fold_bias (fp64, rounded once).
// grid (ceil(w * C / 2 / 256), bands of TH source rows, images) through fd_xcd_image_map; block 256.  Any h, w >= 1 (on a 1 x 1 source every up-pixel is
// the one source value and most taps fall outside).  C % 2 == 0.
//
// fd_head_bilinear rests on: the 1 x 1 convolution and the folded BatchNorm are affine and the bilinear weights sum to 1, so
// s pw(up(x)) + t = up(s pw(x) + t) -- only the activation does not commute.  A workgroup computes the pre-activation z = w . x + t for a 16 x 16 source
// tile plus a one-pixel halo (18 x 18 floats of LDS; halo coordinates are clamped into the map, which IS the interpolation's border rule) with fp32
// weights -- 8 lanes per halo pixel, 16 bytes of channels each, a 3-step shuffle sum, as fd_head_pw1: a wave's loads are dense runs -- and after one barrier every work-item interpolates (columns, then rows), activates and writes the 2 x 2 quad of its source pixel: a quarter of
// the dot products, and no Cin-channel full-size tensor.  A wave covers four tile rows: its stores are runs of 32 floats.  Known difference: with a
// non-finite input the commuted order can differ from the reference's (Inf * w of mixed sign inside one dot product against separately interpolated
// channels); finite inputs agree to rounding.  grid (ceil(w / 16), ceil(h / 16), images); block 256.  Cin % 4 == 0.
#pragma once
#include "fd_device.h"

// a lane's two channels in the storage type T <-> fp32
__device__ __forceinline__ fd_f32x2 fd_dwb_ld2(const float *p) { return *reinterpret_cast<const fd_f32x2 *>(p); }
__device__ __forceinline__ fd_f32x2 fd_dwb_ld2(const fd_half *p)
{
    typedef _Float16 fd_h2_ __attribute__((ext_vector_type(2)));
    const fd_h2_ h = *reinterpret_cast<const fd_h2_ *>(p);
    fd_f32x2 r = {(float)h.x, (float)h.y};
    return r;
}
__device__ __forceinline__ fd_f32x2 fd_dwb_ld2(const fd_bf16 *p)
{
    const unsigned d = *reinterpret_cast<const unsigned *>(p);
    fd_f32x2 r = {__builtin_bit_cast(float, d << 16), __builtin_bit_cast(float, d & 0xffff0000u)};
    return r;
}
__device__ __forceinline__ void fd_dwb_st2(float *p, fd_f32x2 v) { *reinterpret_cast<fd_f32x2 *>(p) = v; }
__device__ __forceinline__ void fd_dwb_st2(fd_half *p, fd_f32x2 v) { *reinterpret_cast<unsigned *>(p) = fd_pack2(fd_half{}, v.x, v.y); }
__device__ __forceinline__ void fd_dwb_st2(fd_bf16 *p, fd_f32x2 v) { *reinterpret_cast<unsigned *>(p) = fd_pack2(fd_bf16{}, v.x, v.y); }

// one interpolation step: 3/4 major + 1/4 minor (the product with 1/4 is exact: one rounding)
__device__ __forceinline__ float fd_dwb_mix(float major, float minor) { return fmaf(0.75f, major, 0.25f * minor); }
__device__ __forceinline__ fd_f32x2 fd_dwb_mix(fd_f32x2 major, fd_f32x2 minor)
{
    fd_f32x2 r = {fd_dwb_mix(major.x, minor.x), fd_dwb_mix(major.y, minor.y)};
    return r;
}
// up index 2 y + U from the source window s[0 .. 2R] = source y-R .. y+R: window indices of the 3/4 (major) and the 1/4 (minor) operand
template <int U, int R> struct fd_dwb_tap {
    static constexpr int m = U >= 0 ? U / 2 : -((1 - U) / 2);                // floor(U / 2)
    static constexpr bool even = (U - 2 * m) == 0;
    static constexpr int major = m + R, minor = even ? m - 1 + R : m + 1 + R;
    static_assert(major >= 0 && major <= 2 * R && minor >= 0 && minor <= 2 * R, "the window covers every up index of the quad");
};

template <typename T, int K, int ACT>
__global__ void __launch_bounds__(256)
fd_dwb_rows(const T *__restrict__ src, const float *__restrict__ wp, const float *__restrict__ bias, T *__restrict__ out, int H, int W, int C, int TH)
{
    static_assert(K == 3 || K == 5, "windows exist for k = 3 and k = 5");
    constexpr int P = (K - 1) / 2, R = P, NW = 2 * R + 1, NU = K + 1;     // NW source rows / columns -> NU up rows / columns
    const int CG = C >> 1;
    const fd_blk3 blk = fd_xcd_image_map();
    const int q = blk.x * 256 + (int)threadIdx.x;
    if (q >= W * CG) return;
    const int x = q / CG, cg = q - x * CG;
    const int n = blk.z;
    const int r0 = blk.y * TH;
    const int r1 = (r0 + TH < H) ? r0 + TH : H;
    fd_f32x2 w[K * K];
#pragma unroll
    for (int t = 0; t < K * K; ++t) w[t] = fd_dwb_ld2(wp + (long)t * C + cg * 2);
    const fd_f32x2 b2 = fd_dwb_ld2(bias + cg * 2);
    const T *img = src + (long)n * H * W * C + cg * 2;
    int xc[NW];                                              // source columns x-R .. x+R clamped into the map: the replicated border of the interpolation
#pragma unroll
    for (int ci = 0; ci < NW; ++ci) { const int v = x - R + ci; xc[ci] = v < 0 ? 0 : (v >= W ? W - 1 : v); }
    const bool okl = x >= 1, okr = x + 1 < W;               // up columns 2x-2, 2x-1 / 2x+2, 2x+3 lie inside the upsampled map
    const fd_f32x2 zero = {0.f, 0.f};
    // one source row (clamped into the map), interpolated horizontally into the NU up columns 2x-P .. 2x+P+1; columns outside the up map are zero (select)
    auto load_row = [&](int iy, fd_f32x2 (&h)[NU]) {
        const int qy = iy < 0 ? 0 : (iy >= H ? H - 1 : iy);
        const T *p = img + (long)qy * W * C;
        fd_f32x2 s[NW];
#pragma unroll
        for (int ci = 0; ci < NW; ++ci) s[ci] = fd_dwb_ld2(p + (long)xc[ci] * C);
        auto col = [&](auto U) {
            typedef fd_dwb_tap<decltype(U)::value, R> TP;
            fd_f32x2 v = fd_dwb_mix(s[TP::major], s[TP::minor]);
            if (decltype(U)::value < 0 && !okl) v = zero;
            if (decltype(U)::value >= 2 && !okr) v = zero;
            h[decltype(U)::value + P] = v;
        };
        col(fd_int<-P>{}); col(fd_int<1 - P>{}); col(fd_int<2 - P>{}); col(fd_int<3 - P>{});
        if constexpr (K == 5) { col(fd_int<2>{}); col(fd_int<3>{}); }
    };
    const int Wo = 2 * W;
    T *o = out + (((long)n * 2 * H + 2 * r0) * Wo + 2 * x) * C + cg * 2;
    fd_f32x2 win[NW][NU];
#pragma unroll
    for (int ri = 0; ri < NW - 1; ++ri) load_row(r0 - R + ri, win[ri]);
    for (int r = r0; r < r1; ++r) {
        load_row(r + R, win[NW - 1]);
        const bool oku = r >= 1, okd = r + 1 < H;          // up rows 2r-2, 2r-1 / 2r+2, 2r+3 lie inside the upsampled map (uniform over the workgroup)
        fd_f32x2 acc[2][2] = {{b2, b2}, {b2, b2}};
        auto up_row = [&](auto U) {
            constexpr int u = decltype(U)::value + P;        // up row 2r - P + u
            typedef fd_dwb_tap<decltype(U)::value, R> TP;
            if (decltype(U)::value < 0 && !oku) return;      // zero padding of the upsampled map: the row contributes nothing
            if (decltype(U)::value >= 2 && !okd) return;
            fd_f32x2 v[NU];
#pragma unroll
            for (int j = 0; j < NU; ++j) v[j] = fd_dwb_mix(win[TP::major][j], win[TP::minor][j]);
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const int ky = u - a;
                if (ky < 0 || ky >= K) continue;
#pragma unroll
                for (int b = 0; b < 2; ++b)
#pragma unroll
                    for (int kx = 0; kx < K; ++kx) {
                        acc[a][b].x = fmaf(v[b + kx].x, w[ky * K + kx].x, acc[a][b].x);
                        acc[a][b].y = fmaf(v[b + kx].y, w[ky * K + kx].y, acc[a][b].y);
                    }
            }
        };
        up_row(fd_int<-P>{}); up_row(fd_int<1 - P>{}); up_row(fd_int<2 - P>{}); up_row(fd_int<3 - P>{});
        if constexpr (K == 5) { up_row(fd_int<2>{}); up_row(fd_int<3>{}); }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                fd_f32x2 v = {fd_act<ACT>(acc[a][b].x), fd_act<ACT>(acc[a][b].y)};
                fd_dwb_st2(o + ((long)a * Wo + b) * C, v);
            }
        o += 2 * (long)Wo * C;
#pragma unroll
        for (int ri = 0; ri < NW - 1; ++ri)
#pragma unroll
            for (int j = 0; j < NU; ++j) win[ri][j] = win[ri + 1][j];
    }
}

#define FD_HEADB_TILE 16
template <typename T, int ACT>
__global__ void __launch_bounds__(256)
fd_head_bilinear(const T *__restrict__ in, const float *__restrict__ wp, const float *__restrict__ bias, float *__restrict__ y, int h, int w, int Cin)
{
    constexpr int TS = FD_HEADB_TILE, HS = TS + 2;           // tile side, tile + halo side
    __shared__ float z[HS * HS];
    const int n = (int)blockIdx.z;
    const int ty0 = (int)blockIdx.y * TS, tx0 = (int)blockIdx.x * TS;
    const T *img = in + (long)n * h * w * Cin;
    const float t = bias[0];
    // z: 8 lanes share one halo pixel (16-byte channel groups: a wave reads 8 adjacent pixels' channels as dense runs, as fd_head_pw1), a 3-step
    // shuffle reduces the dot product.  32 pixels per pass; the trip count is the same for every work-item (the shuffles are wave-wide)
    const int l8 = (int)threadIdx.x & 7, slot = (int)threadIdx.x >> 3;
    for (int e0 = 0; e0 < HS * HS; e0 += 32) {
        const int e = e0 + slot;
        const int ec = e < HS * HS ? e : HS * HS - 1;
        const int hy = ec / HS, hx = ec - hy * HS;
        int gy = ty0 - 1 + hy, gx = tx0 - 1 + hx;             // clamped into the map: loads stay inside it, and the halo holds the replicated border
        gy = gy < 0 ? 0 : (gy >= h ? h - 1 : gy);
        gx = gx < 0 ? 0 : (gx >= w ? w - 1 : gx);
        const T *p = img + ((long)gy * w + gx) * Cin;
        float s = 0.0f;
        for (int c = l8 * 4; c < Cin; c += 32) {
            const fd_f32x4 v = fd_ld4(p + c), k4 = fd_ld4(wp + c);
            s = fmaf(v.x, k4.x, s); s = fmaf(v.y, k4.y, s); s = fmaf(v.z, k4.z, s); s = fmaf(v.w, k4.w, s);
        }
        s += __shfl_xor(s, 1);
        s += __shfl_xor(s, 2);
        s += __shfl_xor(s, 4);
        if (l8 == 0 && e < HS * HS) z[e] = s + t;
    }
    __syncthreads();
    const int ly = (int)threadIdx.x / TS, lx = (int)threadIdx.x % TS;
    const int sy = ty0 + ly, sx = tx0 + lx;
    if (sy >= h || sx >= w) return;
    float c0[3], c1[3];                                      // up columns 2 sx and 2 sx + 1 of source rows sy-1, sy, sy+1
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float *row = z + (ly + i) * HS + lx;           // row[0..2] = source columns sx-1, sx, sx+1
        c0[i] = fd_dwb_mix(row[1], row[0]);
        c1[i] = fd_dwb_mix(row[1], row[2]);
    }
    float *o = y + (((long)n * 2 * h + 2 * sy) * 2 * (long)w + 2 * sx);
    const fd_f32x2 top = {fd_act<ACT>(fd_dwb_mix(c0[1], c0[0])), fd_act<ACT>(fd_dwb_mix(c1[1], c1[0]))};
    const fd_f32x2 bot = {fd_act<ACT>(fd_dwb_mix(c0[1], c0[2])), fd_act<ACT>(fd_dwb_mix(c1[1], c1[2]))};
    *reinterpret_cast<fd_f32x2 *>(o) = top;
    *reinterpret_cast<fd_f32x2 *>(o + 2 * w) = bot;
}
