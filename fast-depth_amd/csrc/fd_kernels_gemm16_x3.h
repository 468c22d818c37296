// fd_kernels_gemm16_x3.h -- the K loop of the split-bf16 form of fd_pw_gemm16_f32 (template parameter X3): the fp32 product on
// v_mfma_f32_16x16x32_bf16.
//
// An fp32 number is exactly the sum of three bf16 numbers, a = a_hi + a_mid + a_lo (8 significand bits each).  Of the nine partial products
// of a * w the six of relative weight >= 2^-16,
//     a_hi w_hi,  a_hi w_mid,  a_hi w_lo,  a_mid w_hi,  a_mid w_mid,  a_lo w_hi,
// accumulated in fp32 reproduce the fp32 product to fp32 rounding (tools/x3_numerics.py).  Six bf16 MFMAs of 16 cycles
// and depth 32 replace the eight fp32 MFMAs of 32 cycles and depth 4 that a SIMD issues per row tile and 32-deep K tile: 96 matrix-pipe cycles
// instead of 256.
//
// Operands (written once: the weights at pack time, the activations by the kernel that produces them):
//   Wp  [3][N][K32]  bf16   planes hi / mid / lo of the folded weights, K padded with zeros to K32 (a multiple of 32)
//   Ap  [K32/32][3][M][32]  bf16   planes hi / mid / lo of A, K padded with zeros to K32, K-tile-major: the 16 rows of an LDS-DMA piece are 1 KiB contiguous
//       (plane-major rows [3][M][K32] measured slower: DESIGN.md Appendix A, r08)
// LDS stage (one 32-deep K tile): 3 (BM + 64) rows of 64 bytes -- A plane 0, 1, 2 (BM rows each), then weight plane 0, 1, 2 (64 rows each) --
// filled by LDS-DMA pieces of 16 rows (lane l: row l >> 2, 16-byte chunk l & 3).  A lane's 16-byte chunk IS its MFMA operand (8 consecutive k):
// fragment reads are ds_read_b128 of row l & 15, chunk l >> 4.  Swizzle: chunk' = chunk ^ swz((row >> 2) & 3), swz = {0, 2, 3, 1}.  ds_read_b128 is
// served in the 16-lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, ...: rows 0-3 and 12-15 with chunk c beside rows 4-11 with chunk c ^ 1.  Rows
// r and r + 4 share their banks, so the four row quads of a group need four different chunk' -- {swz 0, swz 3, 1 ^ swz 1, 1 ^ swz 2} = {0, 1, 3, 2}
// and {swz 1, swz 2, 1 ^ swz 0, 1 ^ swz 3} = {2, 3, 1, 0}: conflict-free (the plain  chunk ^ (row >> 2)  gives {0, 3, 0, 3}: two-way conflicts).
//
// Roles.  Waves w and w + 4 share a SIMD and the 16 output columns wn = w & 3 of all TM row tiles, as in the fp32 form, but they split the six
// PRODUCTS, not K; the partial sums meet in the epilogue exactly as the two k-halves of the fp32 form do.  Consecutive MFMAs on one accumulator are TM
// MFMAs apart.
//   leader (w < 4): a_hi w_hi, and all the LDS-DMA;   follower: a_hi {w_mid, w_lo}, a_mid {w_hi, w_mid}, a_lo w_hi
// The matrix pipe is shared by the two waves whatever the split, and the K loop is bound by the leaders' LDS-DMA issue: the 3 + 3 split (leader a_hi {w_hi,
// w_mid, w_lo}) measured equally fast.  1 + 5 keeps every small product out of the accumulator that holds
// a_hi w_hi -- added there, each would be rounded at the magnitude of the large sum; kept apart they meet it once, in the epilogue.
// Registers: each wave double-buffers ONE plane of a tile (2 x TM fragments):
//   leader    behind barrier k: MFMAs of hi(k-1) while it reads hi(k) and its weight fragments of tile k
//   follower  hi phase of tile k while it reads mid(k); mid phase while it reads lo(k); barrier k+1; lo phase while it reads hi(k+1) and the weight
//             fragments of tile k+1 -- the two buffers swap roles from tile to tile
// Barrier k says "tile k has landed, and every read of tile k-1 has completed" (each wave waits for its own LDS reads before it): one barrier per
// K tile; behind it the stage of tile k-1 takes the LDS-DMA of tile k + STAGES - 1.
#pragma once
#include "fd_device.h"

__device__ __forceinline__ int fd_g16_x3_swz(int q) { return (0x78 >> (2 * q)) & 3; }      // {0, 2, 3, 1}

// Weight planes [3][N][K32] from the folded fp32 weights wf[N][K32] (fd_pack_fold: rows zero-padded to K32), once per fd_plan_pack_weights.  Split by
// TRUNCATION toward zero: every part carries the sign of w and hi + mid + lo == w exactly.  A part that comes out as zero although w != 0 becomes
// copysign(2^-120, w), a normal bf16 far below anything fp32 can resolve next to a product with w: with it (+-Inf) * w has the class and sign it has in
// fp32 in EVERY partial product (never the NaN of Inf * 0).  w == 0 gives three zeros, a non-finite w gives (w, 0, 0).
static __global__ void __launch_bounds__(256) fd_pack_x3_planes(const float *__restrict__ wf, unsigned short *__restrict__ planes, long total)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const float w = wf[idx];
    const unsigned u = __builtin_bit_cast(unsigned, w);
    unsigned short q[3] = {(unsigned short)(u >> 16), 0, 0};
    if ((u & 0x7f800000u) != 0x7f800000u && w != 0.0f) {
        float r = w - fd_bf16_to_f32(q[0]);
        q[1] = (unsigned short)(__builtin_bit_cast(unsigned, r) >> 16);
        r -= fd_bf16_to_f32(q[1]);
        q[2] = (unsigned short)(__builtin_bit_cast(unsigned, r) >> 16);
        const unsigned short filler = (unsigned short)(((u >> 16) & 0x8000u) | 0x0380u);      // copysign(2^-120, w)
#pragma unroll
        for (int i = 0; i < 3; ++i) if ((q[i] & 0x7fffu) == 0) q[i] = filler;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) planes[(long)i * total + idx] = q[i];
}

template <int TM, int STAGES> struct fd_g16_x3_geom {
    static constexpr int BM = TM * 16, BN = 64;
    static constexpr int RT = 3 * (BM + BN);                 // 64-byte rows per stage
    static constexpr int STAGE_B = RT * 64;                  // bytes per stage
    static constexpr int NP = RT / 16;                       // LDS-DMA pieces (1 KiB) per stage
    static constexpr size_t ring_bytes = (size_t)STAGES * STAGE_B;
};

template <int TM, int STAGES>
__device__ __forceinline__ void fd_g16_x3_kloop(const unsigned char *__restrict__ Ap, const unsigned char *__restrict__ Wp, unsigned char *ring, fd_f32x4 (&acc_io)[TM],
                                                long m0, int n0, int M, int N, int K32, long long *stamp)
{
    static_assert(STAGES == 3 || STAGES == 4, "the landed-tile waits are written for 3 or 4 stages");
    typedef fd_g16_x3_geom<TM, STAGES> G;
    constexpr int BM = G::BM, STAGE_B = G::STAGE_B, NP = G::NP;
    constexpr int NLW = 4;                                   // waves that issue LDS-DMA: the leaders
    constexpr int RG = (NP + NLW - 1) / NLW;                 // pieces per issuing wave and K tile (a wave without an own piece in the last round repeats its first)
    constexpr int NPL = 1;                                   // products of the leader
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wn = wave & 3;
    const bool leader = wave < 4;
    const int w_u = FD_UNIFORM(wn);
    const int T = K32 / 32;
    fd_f32x4 acc[TM];                                        // (a local copy: the caller's array keeps constant indices in its epilogue)
#pragma unroll
    for (int i = 0; i < TM; ++i) acc[i] = acc_io[i];

    // ---- LDS-DMA sources: per-lane byte offsets are loop-invariant, the K tile adds a wave-uniform stride ----
    unsigned src_off[RG];
    const int csrc = ((lane & 3) ^ fd_g16_x3_swz((lane >> 4) & 3)) * 16, r16 = lane >> 2;
#pragma unroll
    for (int i = 0; i < RG; ++i) {
        int g = w_u + NLW * i;
        if (g >= NP) g = w_u;
        if (g < 3 * TM) {
            const int p = g / TM, it = g - p * TM;
            long row = m0 + it * 16 + r16;
            if (row > M - 1) row = M - 1;
            src_off[i] = (unsigned)(((long)p * M + row) * 64 + csrc);
        } else {
            const int gw = g - 3 * TM, p = gw >> 2;
            int colw = n0 + (gw & 3) * 16 + r16;
            if (colw > N - 1) colw = N - 1;
            src_off[i] = (unsigned)(((long)p * N + colw) * (K32 * 2) + csrc);
        }
    }
    const size_t a_tstride = (size_t)3 * M * 64;
    auto piece = [&](int t, int i) {
        int g = w_u + NLW * i;
        if (g >= NP) g = w_u;
        const unsigned char *base = g < 3 * TM ? Ap + (size_t)t * a_tstride : Wp + (size_t)t * 64;
        fd_glds16(reinterpret_cast<const float *>(base + src_off[i]), reinterpret_cast<float *>(ring + (t % STAGES) * STAGE_B + g * 1024));
    };
    // tile k has landed: the tiles up to min(k + STAGES - 2, T - 1) have been issued, RG pieces each, and vector-memory operations complete in order
    auto wait_landed = [&](int k) {
        const int younger = (k + STAGES - 2 < T - 1 ? k + STAGES - 2 : T - 1) - k;
        if (younger >= 2) fd_wait_vmcnt<2 * RG>(); else if (younger == 1) fd_wait_vmcnt<RG>(); else fd_wait_vmcnt<0>();
    };

    // ---- fragment offsets (bytes) within a stage ----
    const int fo = (lane & 15) * 64 + (((lane >> 4) ^ fd_g16_x3_swz((lane & 15) >> 2)) << 4);
    const int wo = (3 * BM + wn * 16) * 64 + fo;
    auto ld_a = [&](const unsigned char *st, int p, int i) { return *reinterpret_cast<const fd_u16x8 *>(st + (p * BM + i * 16) * 64 + fo); };
    auto ld_w = [&](const unsigned char *st, int p) { return *reinterpret_cast<const fd_u16x8 *>(st + p * (64 * 64) + wo); };

    if (leader) {
#pragma unroll
        for (int s = 0; s < STAGES - 1; ++s)
            if (s < T) {
#pragma unroll
                for (int i = 0; i < RG; ++i) piece(s, i);
            }
        fd_u16x8 fa[2][TM], fw[2][NPL];
        wait_landed(0);
        fd_block_barrier();                                  // barrier 0
        if (STAGES - 1 < T) {
#pragma unroll
            for (int i = 0; i < RG; ++i) piece(STAGES - 1, i);
        }
#pragma unroll
        for (int i = 0; i < TM; ++i) fa[0][i] = ld_a(ring, 0, i);
#pragma unroll
        for (int p = 0; p < NPL; ++p) fw[0][p] = ld_w(ring, p);
#ifdef FD_GEMM16_PROBE
        if (stamp && tid == 0) *stamp = clock64();
#else
        (void)stamp;
#endif
#ifndef FD_EMU
        __builtin_amdgcn_s_setprio(1);
#endif
        auto mfmas = [&](auto par, const unsigned char *nx, int k, bool do_dma, bool do_frags) __attribute__((always_inline)) {
            constexpr int P = decltype(par)::value, NM = NPL * TM, NL = RG + TM + NPL;
#pragma unroll
            for (int idx = 0; idx < NM; ++idx) {
                const int p = idx / TM, i = idx % TM;
                acc[i] = fd_mfma_bf16_16x16x32(fa[P][i], fw[P][p], acc[i]);
#pragma unroll
                for (int l = idx * NL / NM; l < (idx + 1) * NL / NM; ++l) {
                    if (l < RG) { if (do_dma) piece(k + STAGES - 1, l); }
                    else if (l < RG + TM) { if (do_frags) fa[1 - P][l - RG] = ld_a(nx, 0, l - RG); }
                    else { if (do_frags) fw[1 - P][l - RG - TM] = ld_w(nx, l - RG - TM); }
                }
            }
        };
        auto lstep = [&](auto par, int k) __attribute__((always_inline)) {        // behind barrier k: the MFMAs of tile k - 1
            wait_landed(k);
            fd_block_barrier_lds();
            mfmas(par, ring + (k % STAGES) * STAGE_B, k, k + STAGES - 1 < T, true);
        };
        for (int k = 1; k < T; k += 2) {
            lstep(fd_int<0>{}, k);
            if (k + 1 < T) lstep(fd_int<1>{}, k + 1);
        }
        if ((T - 1) & 1) mfmas(fd_int<1>{}, ring, 0, false, false); else mfmas(fd_int<0>{}, ring, 0, false, false);
#ifndef FD_EMU
        __builtin_amdgcn_s_setprio(0);
#endif
    } else {
        // the follower of a leader that takes a_hi * w_hi alone: five products in three phases on two fragment buffers whose roles swap from tile to tile --
        //   hi phase   a_hi * {w_mid, w_lo} of tile k   (buffer P)      while it reads mid(k) into buffer 1 - P
        //   mid phase  a_mid * {w_hi, w_mid}            (buffer 1 - P)  while it reads lo(k) into buffer P;  then barrier k + 1
        //   lo phase   a_lo * w_hi                      (buffer P)      while it reads hi(k + 1) into buffer 1 - P and the three weight fragments of tile k + 1
        fd_u16x8 fb[2][TM], wq[2][3];
        fd_block_barrier();                                  // barrier 0
#pragma unroll
        for (int i = 0; i < TM; ++i) fb[0][i] = ld_a(ring, 0, i);
#pragma unroll
        for (int p = 0; p < 3; ++p) wq[0][p] = ld_w(ring, p);
        auto fstep = [&](auto par, int k) __attribute__((always_inline)) {
            constexpr int P = decltype(par)::value;
            const unsigned char *cur = ring + (k % STAGES) * STAGE_B, *nx = ring + ((k + 1) % STAGES) * STAGE_B;
            const bool more = k + 1 < T;
#pragma unroll
            for (int idx = 0; idx < 2 * TM; ++idx) {
                const int i = idx % TM;
                acc[i] = fd_mfma_bf16_16x16x32(fb[P][i], wq[P][idx < TM ? 1 : 2], acc[i]);
                if (idx & 1) fb[1 - P][idx >> 1] = ld_a(cur, 1, idx >> 1);
            }
#pragma unroll
            for (int idx = 0; idx < 2 * TM; ++idx) {
                const int i = idx % TM;
                acc[i] = fd_mfma_bf16_16x16x32(fb[1 - P][i], wq[P][idx < TM ? 0 : 1], acc[i]);
                if (idx & 1) fb[P][idx >> 1] = ld_a(cur, 2, idx >> 1);
            }
            if (more) fd_block_barrier_lds();                // barrier k + 1
#pragma unroll
            for (int idx = 0; idx < TM; ++idx) {
                acc[idx] = fd_mfma_bf16_16x16x32(fb[P][idx], wq[P][0], acc[idx]);
                if (more) fb[1 - P][idx] = ld_a(nx, 0, idx);
                if (more && idx < 3) wq[1 - P][idx] = ld_w(nx, idx);
            }
        };
        for (int k = 0; k < T; k += 2) {
            fstep(fd_int<0>{}, k);
            if (k + 1 < T) fstep(fd_int<1>{}, k + 1);
        }
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) acc_io[i] = acc[i];
}
