// fd_kernels_dws.h -- the two primitives of the reference's pixel-shuffle decoder ShuffleConv(k, dw=True) (models.py:296-333):
//
//   fd_dws_rows<T, K, ACT>    depthwise k x k convolution (k = 3 or 5, stride 1, padding (k-1)/2) + folded BatchNorm + activation ON THE 2x PIXEL
//                             SHUFFLE of its producer's output: the shuffled tensor is never written, the kernel reads through the index map
//   fd_head_shuffle<T, ACT>   pointwise Cin -> 4 + folded BatchNorm + activation whose four outputs per pixel are written as the 2 x 2 quad of
//                             the fp32 NCHW network output: the last pixel shuffle happens in the store
//
// Index map (F.pixel_shuffle(., 2) in NHWC): with src = [B][h][w][4C], the convolution's input is in[n][2y+i][2x+j][c] = src[n][y][x][4c + 2i + j],
// a [B][2h][2w][C] map.  Output pixel (2y+a, 2x+b) reads input rows 2y+a-p .. 2y+a+p, p = (k-1)/2: for a in {0, 1} and both k these lie in source
// rows y-1 .. y+1 (k = 5: input rows 2y-2 .. 2y+3; k = 3: 2y-1 .. 2y+2), columns alike -- the 2 x 2 output quad of source pixel (y, x) is a function
// of the 3 x 3 source window around it.  Window pixel (ri, ci) (source row y-1+ri, column x-1+ci), sub-position (i, j) meets tap
// (ky, kx) = (2 ri - 2 + i - a + p, 2 ci - 2 + j - b + p) where that is inside the kernel: every tap of every output meets exactly one real input
// (k^2 multiply-adds per output; nothing to save by parity, unlike the transposed convolution of fd_kernels_dwt.h).  A source pixel outside
// the map stands for four input pixels outside the map: the zero padding is a select on whole source pixels.
//
// fd_dws_rows is the register-window form of fd_dwt_rows: no LDS, no barrier.  Work-item q = x * (C / G) + cg owns source column x and G adjacent
// OUTPUT channels = 4 G contiguous source channels = ONE 16-byte load per window pixel: G = 1 in fp32, G = 2 in the 16-bit plans.  It walks down
// the source rows of its band with the three-row window and its channels' k^2 folded fp32 taps in registers; every step loads the window's new
// bottom row (3 loads) and emits output rows 2y and 2y+1 (4 pixels x G channels, each a full k^2 fmaf chain started from the folded bias).
// Consecutive lanes take consecutive channel groups, then the next column: a wave's loads are contiguous, and its stores (4 bytes per lane) cover
// runs of C elements.  Loads are issued at an address clamped into the map.
// grid (ceil(w * C / G / 256), bands of TH source rows, images) through fd_xcd_image_map; block 256.  Any h, w >= 1 (a 1 x 1 source makes a 2 x 2
// map on which most taps fall outside).  Channel constraint: C >= 1 in fp32 plans, C % 2 == 0 in 16-bit plans (C = the layer's cin == cout; the
// producer has 4 C channels).
//
// fd_head_shuffle: one work-item per source pixel (consecutive lanes = consecutive x); Cin values (4 per load), four fp32 dot products with the
// fp32 weights wp[Cin][4] (fd_pack_fold's tap-major layout), + bias, activation, two 8-byte stores into rows 2y and 2y+1 of y: a wave writes two
// contiguous runs.  Cin % 4 == 0.
#pragma once
#include "fd_device.h"

// a lane's 4 G source channels and G output channels in the storage type T
template <typename T> struct fd_dws_lane {                   // 16-bit storage: 8 source channels (16 bytes), 2 output channels (4 bytes)
    static constexpr int G = 2;
    typedef fd_f32x8 vec;
    static __device__ __forceinline__ vec ld(const T *p) { return fd_lane<T, 8>::ld(p); }
    static __device__ __forceinline__ vec zero() { return fd_zero8(); }
    static __device__ __forceinline__ void ldw(const float *p, float (&w)[G]) { const fd_f32x2 v = *reinterpret_cast<const fd_f32x2 *>(p); w[0] = v.x; w[1] = v.y; }
    static __device__ __forceinline__ void st(T *p, const float (&v)[G]) { *reinterpret_cast<unsigned *>(p) = fd_pack2(T{}, v[0], v[1]); }
};
template <> struct fd_dws_lane<float> {                      // fp32: 4 source channels (16 bytes), 1 output channel
    static constexpr int G = 1;
    typedef fd_f32x4 vec;
    static __device__ __forceinline__ vec ld(const float *p) { return fd_ld4(p); }
    static __device__ __forceinline__ vec zero() { return fd_zero4(); }
    static __device__ __forceinline__ void ldw(const float *p, float (&w)[G]) { w[0] = *p; }
    static __device__ __forceinline__ void st(float *p, const float (&v)[G]) { *p = v[0]; }
};

template <typename T, int K, int ACT>
__global__ void __launch_bounds__(256)
fd_dws_rows(const T *__restrict__ src, const float *__restrict__ wp, const float *__restrict__ bias, T *__restrict__ out, int H, int W, int C, int TH)
{
    static_assert(K == 3 || K == 5, "the 3 x 3 source window covers k = 3 and k = 5");
    constexpr int P = (K - 1) / 2;
    typedef fd_dws_lane<T> LN;
    constexpr int G = LN::G;
    typedef typename LN::vec vec;
    const int CG = C / G, CS = 4 * C;                        // channel groups per pixel; source channels
    const fd_blk3 blk = fd_xcd_image_map();
    const int q = blk.x * 256 + (int)threadIdx.x;
    if (q >= W * CG) return;
    const int x = q / CG, cg = q - x * CG;
    const int n = blk.z;
    const int r0 = blk.y * TH;
    const int r1 = (r0 + TH < H) ? r0 + TH : H;
    float w[K * K][G], b[G];
#pragma unroll
    for (int t = 0; t < K * K; ++t) LN::ldw(wp + (long)t * C + cg * G, w[t]);
    LN::ldw(bias + cg * G, b);
    const T *img = src + (long)n * H * W * CS + cg * 4 * G;
    const bool okl = x >= 1, okr = x + 1 < W;
    const int xl = okl ? x - 1 : x, xr = okr ? x + 1 : x;    // clamped: the loads are always issued inside the map, the padding is a select
    auto load_row = [&](int iy, vec (&v)[3]) {
        const bool oky = iy >= 0 && iy < H;
        const int qy = iy < 0 ? 0 : (iy >= H ? H - 1 : iy);
        const T *p = img + (long)qy * W * CS;
        v[0] = LN::ld(p + (long)xl * CS); if (!(oky && okl)) v[0] = LN::zero();
        v[1] = LN::ld(p + (long)x * CS); if (!oky) v[1] = LN::zero();
        v[2] = LN::ld(p + (long)xr * CS); if (!(oky && okr)) v[2] = LN::zero();
    };
    const int Wo = 2 * W;
    T *o = out + (((long)n * 2 * H + 2 * r0) * Wo + 2 * x) * C + cg * G;
    vec win[3][3];
    load_row(r0 - 1, win[0]);
    load_row(r0, win[1]);
    for (int r = r0; r < r1; ++r) {
        load_row(r + 1, win[2]);
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int bb = 0; bb < 2; ++bb) {
                float acc[G];
#pragma unroll
                for (int g = 0; g < G; ++g) acc[g] = b[g];
#pragma unroll
                for (int ri = 0; ri < 3; ++ri)
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const int ky = 2 * ri - 2 + i - a + P;    // window row ri, sub-row i is input row 2 (r - 1 + ri) + i
                        if (ky < 0 || ky >= K) continue;
#pragma unroll
                        for (int ci = 0; ci < 3; ++ci)
#pragma unroll
                            for (int j = 0; j < 2; ++j) {
                                const int kx = 2 * ci - 2 + j - bb + P;
                                if (kx < 0 || kx >= K) continue;
#pragma unroll
                                for (int g = 0; g < G; ++g) acc[g] = fmaf(win[ri][ci][4 * g + 2 * i + j], w[ky * K + kx][g], acc[g]);
                            }
                    }
#pragma unroll
                for (int g = 0; g < G; ++g) acc[g] = fd_act<ACT>(acc[g]);
                LN::st(o + ((long)a * Wo + bb) * C, acc);
            }
        o += 2 * (long)Wo * C;
#pragma unroll
        for (int ci = 0; ci < 3; ++ci) { win[0][ci] = win[1][ci]; win[1][ci] = win[2][ci]; }
    }
}

template <typename T, int ACT>
__global__ void __launch_bounds__(256)
fd_head_shuffle(const T *__restrict__ in, const float *__restrict__ wp, const float *__restrict__ bias, float *__restrict__ y, long npix, int h, int w, int Cin)
{
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= npix) return;
    fd_f32x4 s = fd_zero4();
    const T *p = in + g * Cin;
    for (int c = 0; c < Cin; c += 4) {
        const fd_f32x4 v = fd_ld4(p + c);
        const fd_f32x4 q0 = fd_ld4(wp + 4 * c), q1 = fd_ld4(wp + 4 * c + 4), q2 = fd_ld4(wp + 4 * c + 8), q3 = fd_ld4(wp + 4 * c + 12);
        s.x = fmaf(v.x, q0.x, s.x); s.y = fmaf(v.x, q0.y, s.y); s.z = fmaf(v.x, q0.z, s.z); s.w = fmaf(v.x, q0.w, s.w);
        s.x = fmaf(v.y, q1.x, s.x); s.y = fmaf(v.y, q1.y, s.y); s.z = fmaf(v.y, q1.z, s.z); s.w = fmaf(v.y, q1.w, s.w);
        s.x = fmaf(v.z, q2.x, s.x); s.y = fmaf(v.z, q2.y, s.y); s.z = fmaf(v.z, q2.z, s.z); s.w = fmaf(v.z, q2.w, s.w);
        s.x = fmaf(v.w, q3.x, s.x); s.y = fmaf(v.w, q3.y, s.y); s.z = fmaf(v.w, q3.z, s.z); s.w = fmaf(v.w, q3.w, s.w);
    }
    const fd_f32x4 r = fd_act4<ACT>(s + fd_ld4(bias));
    const int ox = (int)(g % w);
    const long t = g / w;
    const int oy = (int)(t % h);
    const long n = t / h;
    float *o = y + ((n * 2 * h + 2 * oy) * 2 * (long)w + 2 * ox);
    const fd_f32x2 top = {r.x, r.y}, bot = {r.z, r.w};       // channel 2 i + j -> output (2y + i, 2x + j)
    *reinterpret_cast<fd_f32x2 *>(o) = top;
    *reinterpret_cast<fd_f32x2 *>(o + 2 * w) = bot;
}
