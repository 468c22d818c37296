// standalone microbench: fd_pw_gemm16_f32 (16x16x4 MFMA, k-split wave pairs, one workgroup per CU) against the 32x32x2 kernel
// on the pointwise shapes of the network (not product code).  usage: gemm16 [shape index | -2: K sweep + ablations | -3: shader clock | -4 [iters]: LDS form vs register form (BREG)
// of the weight fragments on the batch-32 plan's six launch shapes, with the phase table of the probe stamps | -5 [iters]: the plan's form against the split-bf16 form (X3)
// on the batch-32 plan's launch shapes, synthetic planes split on the host, same phase table]
#define FD_GEMM16_PROBE 1
#include "../../fast-depth_amd/csrc/fd_kernels_f32.h"
#include "../../fast-depth_amd/csrc/fd_kernels_gemm16_f32.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <vector>
#include <algorithm>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); exit(1);} } while (0)

static hipEvent_t e0, e1;

template <int WGM,int WGN,int TM,int TN>
float run_old(const float* A, const float* W, const float* bias, float* out, int M, int N, int K, int iters) {
  constexpr int BM=WGM*TM*32, BN=WGN*TN*32;
  int mt=(M+BM-1)/BM, nt=(N+BN-1)/BN; size_t lds = 3*(BM+BN)*32*4;
  if (lds > 65536) CK(hipFuncSetAttribute((const void*)fd_pw_gemm_f32<WGM,WGN,TM,TN,2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  dim3 grid((mt+7)/8*8*nt);
  for (int i=0;i<2;++i) hipLaunchKernelGGL((fd_pw_gemm_f32<WGM,WGN,TM,TN,2>), grid, dim3(64*WGM*WGN), lds, 0, A,W,bias,out,M,N,K,(K+31)/32*32,mt,nt);
  CK(hipEventRecord(e0,0));
  for (int i=0;i<iters;++i) hipLaunchKernelGGL((fd_pw_gemm_f32<WGM,WGN,TM,TN,2>), grid, dim3(64*WGM*WGN), lds, 0, A,W,bias,out,M,N,K,(K+31)/32*32,mt,nt);
  CK(hipEventRecord(e1,0)); CK(hipEventSynchronize(e1)); CK(hipGetLastError());
  float ms; CK(hipEventElapsedTime(&ms,e0,e1)); return ms/iters*1e3f;
}

template <int TM, int S, int ABL = 0>
float run_new(const float* A, const float* W, const float* bias, float* out, int M, int N, int K, int stride, int iters) {
  int mt=(M+stride-1)/stride, nt=(N+63)/64; size_t lds = (size_t)S*(TM*16+64)*32*4;
  CK(hipFuncSetAttribute((const void*)fd_pw_gemm16_f32<TM,S,2,ABL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  dim3 grid((mt+7)/8*8*nt);
  for (int i=0;i<2;++i) hipLaunchKernelGGL((fd_pw_gemm16_f32<TM,S,2,ABL>), grid, dim3(512), lds, 0, A,W,bias,out,M,N,K,(K+31)/32*32,stride,mt,nt, fd_dwfuse{}, fd_g16_train{});
  CK(hipEventRecord(e0,0));
  for (int i=0;i<iters;++i) hipLaunchKernelGGL((fd_pw_gemm16_f32<TM,S,2,ABL>), grid, dim3(512), lds, 0, A,W,bias,out,M,N,K,(K+31)/32*32,stride,mt,nt, fd_dwfuse{}, fd_g16_train{});
  CK(hipEventRecord(e1,0)); CK(hipEventSynchronize(e1)); CK(hipGetLastError());
  float ms; CK(hipEventElapsedTime(&ms,e0,e1)); return ms/iters*1e3f;
}

// the product's launches (batch 32): LDS form (BREG = 0) against the register form of the weight fragments (BREG = 1), with the fused depthwise consumer
// where the plan has one; prints us per launch and the phase table of the probe stamps (mean over the workgroups of the last launch)
struct Phase { float us; double pro, kloop, epi, ghz, exch; };   // exch: the part of the epilogue up to the finished image (partial sums exchanged, before the global stores / the fused consumer)
template <int TM, int FDW, int BREG>
Phase run_form(const float* A, const float* W, const float* bias, float* out, float* dwout, const float* taps, int M, int N, int K, int stride, int fH, int up, int iters, int fS = 1) {
  constexpr int S = 4;
  int mt=(M+stride-1)/stride, nt=(N+63)/64; size_t lds = (size_t)S*(TM*16+(BREG?0:64))*32*4;
  fd_dwfuse fz{};
  if (FDW) {
    fz.w = taps; fz.b = bias; fz.out = dwout; fz.H = fH; fz.W = fH; fz.S = fS; fz.up = up; fz.hi = 6.0f; fz.store_pw = 0;
    const int P = up ? (FDW/2+1)/2 : FDW/2;
    lds = std::max(lds, ((size_t)(stride/(fH*fH))*(fH+2*P)*(fH+2*P)+1)*68*4);
  }
  CK(hipFuncSetAttribute((const void*)fd_pw_gemm16_f32<TM,S,2,0,FDW,0,BREG>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  dim3 grid((mt+7)/8*8*nt);
  for (int i=0;i<3;++i) hipLaunchKernelGGL((fd_pw_gemm16_f32<TM,S,2,0,FDW,0,BREG>), grid, dim3(512), lds, 0, A,W,bias,out,M,N,K,(K+31)/32*32,stride,mt,nt, fz, fd_g16_train{});
  CK(hipEventRecord(e0,0));
  for (int i=0;i<iters;++i) hipLaunchKernelGGL((fd_pw_gemm16_f32<TM,S,2,0,FDW,0,BREG>), grid, dim3(512), lds, 0, A,W,bias,out,M,N,K,(K+31)/32*32,stride,mt,nt, fz, fd_g16_train{});
  CK(hipEventRecord(e1,0)); CK(hipEventSynchronize(e1)); CK(hipGetLastError());
  float ms; CK(hipEventElapsedTime(&ms,e0,e1));
  std::vector<long long> pr(8*grid.x); CK(hipMemcpyFromSymbol(pr.data(), HIP_SYMBOL(fd_gemm16_probe), pr.size()*8));
  Phase ph{ms/iters*1e3f, 0, 0, 0, 0, 0}; double cyc = 0, wall = 0; int n = 0;
  for (unsigned b = 0; b < grid.x; ++b) { const long long* q = &pr[8*b]; if (!q[6] || (int)((b>>3)/nt*8+(b&7)) >= mt) continue;
    ph.exch += (double)(q[1]-q[5]); ph.pro += (double)(q[4]-q[0]); ph.kloop += (double)(q[5]-q[4]); ph.epi += (double)(q[6]-q[5]); cyc += (double)(q[1]-q[0]); wall += (double)(q[3]-q[2]); ++n; }
  ph.pro /= n; ph.kloop /= n; ph.epi /= n; ph.exch /= n; ph.ghz = cyc/wall*0.1;
  return ph;
}

// the split-bf16 form (fd_kernels_gemm16_x3.h): X3 = 13, the one form built (profiles/r08/gemm16_x3_ab.txt also lists the variants that lost -- plane-major A rows,
// all eight waves issuing LDS-DMA, the 3 + 3 split of the products -- which were removed from the kernel after that measurement)
template <int TM, int FDW, int X3, int S>
Phase run_x3(const void* Ap, const void* Wp, const float* bias, float* out, float* dwout, const float* taps, int M, int N, int K, int stride, int fH, int fS, int up, int iters) {
  int mt=(M+stride-1)/stride, nt=(N+63)/64; size_t lds = fd_g16_x3_geom<TM,S>::ring_bytes;
  fd_dwfuse fz{};
  if (FDW) {
    fz.w = taps; fz.b = bias; fz.out = dwout; fz.H = fH; fz.W = fH; fz.S = fS; fz.up = up; fz.hi = 6.0f; fz.store_pw = 0;
    const int P = up ? (FDW/2+1)/2 : FDW/2;
    lds = std::max(lds, ((size_t)(stride/(fH*fH))*(fH+2*P)*(fH+2*P)+1)*68*4);
  }
  auto kern = fd_pw_gemm16_f32<TM,S,2,0,FDW,0,0,X3>;
  CK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  dim3 grid((mt+7)/8*8*nt);
  const float *A = (const float*)Ap, *W = (const float*)Wp;
  for (int i=0;i<3;++i) hipLaunchKernelGGL(kern, grid, dim3(512), lds, 0, A,W,bias,out,M,N,K,(K+31)/32*32,stride,mt,nt, fz, fd_g16_train{});
  CK(hipEventRecord(e0,0));
  for (int i=0;i<iters;++i) hipLaunchKernelGGL(kern, grid, dim3(512), lds, 0, A,W,bias,out,M,N,K,(K+31)/32*32,stride,mt,nt, fz, fd_g16_train{});
  CK(hipEventRecord(e1,0)); CK(hipEventSynchronize(e1)); CK(hipGetLastError());
  float ms; CK(hipEventElapsedTime(&ms,e0,e1));
  std::vector<long long> pr(8*grid.x); CK(hipMemcpyFromSymbol(pr.data(), HIP_SYMBOL(fd_gemm16_probe), pr.size()*8));
  Phase ph{ms/iters*1e3f, 0, 0, 0, 0, 0}; double cyc = 0, wall = 0; int n = 0;
  for (unsigned b = 0; b < grid.x; ++b) { const long long* q = &pr[8*b]; if (!q[6] || (int)((b>>3)/nt*8+(b&7)) >= mt) continue;
    ph.exch += (double)(q[1]-q[5]); ph.pro += (double)(q[4]-q[0]); ph.kloop += (double)(q[5]-q[4]); ph.epi += (double)(q[6]-q[5]); cyc += (double)(q[1]-q[0]); wall += (double)(q[3]-q[2]); ++n; }
  ph.pro /= n; ph.kloop /= n; ph.epi /= n; ph.exch /= n; ph.ghz = cyc/wall*0.1;
  return ph;
}

// host-side splits of an fp32 value into three bf16: activations by round-to-nearest (hi = bf16(a), mid = bf16(a - hi), lo = bf16(a - hi - mid): exact),
// weights by truncation toward zero (every part carries the sign of w; a part that comes out zero although w != 0 becomes copysign(2^-120, w))
static unsigned short bf16_rne(float f) { unsigned u; memcpy(&u,&f,4); u += 0x7fffu + ((u>>16)&1u); return (unsigned short)(u>>16); }
static float bf16_f(unsigned short b) { unsigned u = (unsigned)b<<16; float f; memcpy(&f,&u,4); return f; }
static void split_a(float a, unsigned short p[3]) { p[0] = bf16_rne(a); float r = a - bf16_f(p[0]); p[1] = bf16_rne(r); r -= bf16_f(p[1]); p[2] = bf16_rne(r); }
static void split_w(float w, unsigned short p[3]) {
  unsigned u; float r = w;
  for (int i = 0; i < 3; ++i) { memcpy(&u,&r,4); p[i] = (unsigned short)(u>>16); r -= bf16_f(p[i]); }
  if (w != 0) { memcpy(&u,&w,4); for (int i = 0; i < 3; ++i) if ((p[i] & 0x7fff) == 0) p[i] = (unsigned short)(((u>>16)&0x8000u) | 0x0380u); }
}

static double maxdiff(const float* a, const float* b, size_t n, std::vector<float>& ha, std::vector<float>& hb) {
  ha.resize(n); hb.resize(n);
  CK(hipMemcpy(ha.data(), a, n*4, hipMemcpyDeviceToHost)); CK(hipMemcpy(hb.data(), b, n*4, hipMemcpyDeviceToHost));
  double d = 0, m = 0; for (size_t i=0;i<n;++i) { d = std::max(d, (double)fabsf(ha[i]-hb[i])); m = std::max(m, (double)fabsf(ha[i])); }
  return d / (m > 0 ? m : 1);
}

int main(int argc, char** argv) {
  const int only = argc > 1 ? atoi(argv[1]) : -1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  const size_t maxA = (size_t)401408*128, maxW = 4096*1024, maxO = (size_t)401408*128;
  float *A,*W,*bias,*out,*out2; CK(hipMalloc(&A,maxA*4)); CK(hipMalloc(&W,maxW*4)); CK(hipMalloc(&bias,8192)); CK(hipMalloc(&out,maxO*4)); CK(hipMalloc(&out2,maxO*4));
  std::vector<float> h(maxA); for (auto& v: h) v = (rand()%2001-1000)*1e-3f; CK(hipMemcpy(A,h.data(),maxA*4,hipMemcpyHostToDevice));
  for (auto& v: h) v = (rand()%2001-1000)*2e-4f;
  CK(hipMemcpy(W,h.data(),maxW*4,hipMemcpyHostToDevice)); CK(hipMemcpy(bias,h.data(),8192,hipMemcpyHostToDevice));
  struct S{int M,N,K;}; S shapes[] = {{6272,512,512},{6272,512,256},{1568,1024,1024},{1568,1024,512},{1568,512,1024},{6272,256,512},{25088,256,256},{25088,256,128},{25088,128,256},
                                      {100352,128,128},{100352,128,64},{100352,64,128},{401408,64,32},{401408,32,64},
                                      {12544,408,256},{12544,376,408},{50176,120,256},{200704,56,120},{3136,200,512}};
  std::vector<float> ha, hb;
  if (only == -4) {   // A/B of the two forms on the six launch shapes of the batch-32 fp32 plan
    const int iters = argc > 2 ? atoi(argv[2]) : 50;
    float *dw1, *dw2, *taps; CK(hipMalloc(&dw1,(size_t)6272*1024*4*4)); CK(hipMalloc(&dw2,(size_t)6272*1024*4*4)); CK(hipMalloc(&taps,25*1024*4));
    CK(hipMemcpy(taps,h.data(),25*1024*4,hipMemcpyHostToDevice));
    printf("%-34s %-5s %8s | %9s %9s %9s cycles (GHz) | K loop per K tile\n", "launch", "form", "us", "prologue", "K loop", "epilogue");
    auto show = [&](const char* name, int K, const Phase& a, const Phase& b, double diff) {
      const Phase* f[2] = {&a, &b};
      for (int i = 0; i < 2; ++i)
        printf("%-34s %-5s %8.2f | %9.0f %9.0f %9.0f (%.3f) | %.0f cycles = %.3f us%s\n", name, i ? "BREG" : "LDS", f[i]->us, f[i]->pro, f[i]->kloop, f[i]->epi, f[i]->ghz,
               f[i]->kloop/((K+31)/32), f[i]->kloop/((K+31)/32)/f[i]->ghz*1e-3, i ? (diff == 0 ? "  outputs bitwise equal" : "  OUTPUTS DIFFER") : "");
      fflush(stdout);
    };
#define AB(name, TM, FDW, M, N, K, stride, fH, up, nout) do { \
      CK(hipMemset(out, 0, (size_t)(nout)*4)); CK(hipMemset(out2, 0, (size_t)(nout)*4)); \
      Phase a = run_form<TM,FDW,0>(A,W,bias,FDW?out2:out,out,taps,M,N,K,stride,fH,up,iters); \
      Phase b = run_form<TM,FDW,1>(A,W,bias,FDW?out:out2,out2,taps,M,N,K,stride,fH,up,iters); \
      show(name, K, a, b, maxdiff(out, out2, (size_t)(nout), ha, hb)); } while (0)
    (void)dw1; (void)dw2;
    AB("conv6.3  6272x512x256 TM13 +dw3", 13, 3, 6272, 512, 256, 196, 14, 0, (size_t)6272*512);
    AB("conv7.3  6272x512x512 TM13 +dw3", 13, 3, 6272, 512, 512, 196, 14, 0, (size_t)6272*512);
    AB("conv12.3 1568x1024x512 TM7 +dw3", 7, 3, 1568, 1024, 512, 98, 7, 0, (size_t)1568*1024);
    AB("conv13.3 1568x1024x1024 TM7 +dw5", 7, 5, 1568, 1024, 1024, 98, 7, 0, (size_t)1568*1024);
    AB("dec1.1 1568x512x1024 TM4 +dw5up2", 4, 5, 1568, 512, 1024, 49, 7, 1, (size_t)6272*512);
    AB("dec2.1 6272x256x512 TM7", 7, 0, 6272, 256, 512, 98, 0, 0, (size_t)6272*256);
    AB("dec3.1 25088x128x256 TM13", 13, 0, 25088, 128, 256, 196, 0, 0, (size_t)25088*128);
#undef AB
    return 0;
  }
  if (only == -5) {   // the plan's form (LDS at TM = 13, BREG at TM = 7 / 4) against the split-bf16 form on the launch shapes of the batch-32 fp32 plan
    const int iters = argc > 2 ? atoi(argv[2]) : 50;
    float *taps; CK(hipMalloc(&taps,25*1024*4)); CK(hipMemcpy(taps,h.data(),25*1024*4,hipMemcpyHostToDevice));
    const size_t maxP = (size_t)25088*256;                     // largest M * K of the shapes below
    unsigned short *ApT, *Wp; CK(hipMalloc(&ApT,maxP*6)); CK(hipMalloc(&Wp,(size_t)1024*1024*6));
    std::vector<float> hA(maxA < maxP ? maxA : maxP), hW((size_t)1024*1024);
    CK(hipMemcpy(hA.data(),A,hA.size()*4,hipMemcpyDeviceToHost)); CK(hipMemcpy(hW.data(),W,hW.size()*4,hipMemcpyDeviceToHost));
    std::vector<unsigned short> pt_(maxP*3), pw_((size_t)1024*1024*3);
    auto planes = [&](int M, int N, int K) {                  // A[M][K], W[N][K] (K % 32 == 0) -> planes
      unsigned short q[3];
      for (size_t m = 0; m < (size_t)M; ++m) for (int k = 0; k < K; ++k) { split_a(hA[m*K+k], q);
        for (int p = 0; p < 3; ++p) pt_[(((size_t)(k/32)*3+p)*M+m)*32+k%32] = q[p]; }
      for (size_t n = 0; n < (size_t)N; ++n) for (int k = 0; k < K; ++k) { split_w(hW[n*K+k], q); for (int p = 0; p < 3; ++p) pw_[((size_t)p*N+n)*K+k] = q[p]; }
      CK(hipMemcpy(ApT,pt_.data(),(size_t)M*K*6,hipMemcpyHostToDevice)); CK(hipMemcpy(Wp,pw_.data(),(size_t)N*K*6,hipMemcpyHostToDevice));
    };
    printf("%-36s %-9s %8s | %9s %9s %9s (%s) cycles (GHz) | K loop per K tile | max|y - y_plan| / max|y_plan|\n", "launch", "form", "us", "prologue", "K loop", "epilogue", "of which up to the finished image");
    auto line = [&](const char* name, const char* form, int K, const Phase& f, double diff) {
      printf("%-36s %-9s %8.2f | %9.0f %9.0f %9.0f (%5.0f) (%.3f) | %.0f cycles = %.3f us", name, form, f.us, f.pro, f.kloop, f.epi, f.exch, f.ghz, f.kloop/(K/32), f.kloop/(K/32)/f.ghz*1e-3);
      if (diff >= 0) printf(" | %.2e", diff);
      printf("\n"); fflush(stdout);
    };
#define X3RUN(name, form, TM, FDW, X3, S, AP, M, N, K, stride, fH, fS, up, nout) do { \
      CK(hipMemset(out2, 0, (size_t)(nout)*4)); \
      Phase b = run_x3<TM,FDW,X3,S>(AP,Wp,bias,FDW?out:out2,out2,taps,M,N,K,stride,fH,fS,up,iters); \
      line(name, form, K, b, maxdiff(out, out2, (size_t)(nout), ha, hb)); } while (0)
#define AB5(name, TM, FDW, BREG, S, M, N, K, stride, fH, fS, up, nout) do { \
      planes(M, N, K); CK(hipMemset(out, 0, (size_t)(nout)*4)); \
      Phase a = run_form<TM,FDW,BREG>(A,W,bias,FDW?out2:out,out,taps,M,N,K,stride,fH,up,iters,fS); \
      line(name, BREG ? "f32 BREG" : "f32 LDS", K, a, -1.0); \
      X3RUN(name, "x3 1+5 T", TM, FDW, 13, S, ApT, M, N, K, stride, fH, fS, up, nout); } while (0)
    AB5("conv6.3  6272x512x256 TM13 +dw3", 13, 3, 0, 3, 6272, 512, 256, 196, 14, 1, 0, (size_t)6272*512);
    AB5("conv7-10.3 6272x512x512 TM13 +dw3", 13, 3, 0, 3, 6272, 512, 512, 196, 14, 1, 0, (size_t)6272*512);
    AB5("conv11.3 6272x512x512 TM13 +dw3s2", 13, 3, 0, 3, 6272, 512, 512, 196, 14, 2, 0, (size_t)1568*512);
    AB5("conv12.3 1568x1024x512 TM7 +dw3", 7, 3, 1, 4, 1568, 1024, 512, 98, 7, 1, 0, (size_t)1568*1024);
    AB5("conv13.3 1568x1024x1024 TM7 +dw5", 7, 5, 1, 4, 1568, 1024, 1024, 98, 7, 1, 0, (size_t)1568*1024);
    AB5("dec1.1 1568x512x1024 TM4 +dw5up2", 4, 5, 1, 4, 1568, 512, 1024, 49, 7, 1, 1, (size_t)6272*512);
    AB5("dec2.1 6272x256x512 TM7", 7, 0, 1, 4, 6272, 256, 512, 98, 0, 1, 0, (size_t)6272*256);
    AB5("dec3.1 25088x128x256 TM13", 13, 0, 0, 3, 25088, 128, 256, 196, 0, 1, 0, (size_t)25088*128);
#undef AB5
#undef X3RUN
    return 0;
  }
  if (only == -3) {   // effective shader clock inside the kernel: clock64() ticks per 100 MHz wall tick, main loop only (before the stores)
    for (int abl : {0, 1, 3}) {
      float t = abl == 0 ? run_new<13,4,0>(A,W,bias,out2,6272,512,2048,196,10) : abl == 1 ? run_new<13,4,1>(A,W,bias,out2,6272,512,2048,196,10) : run_new<13,4,3>(A,W,bias,out2,6272,512,2048,196,10);
      std::vector<long long> pr(8*256); CK(hipMemcpyFromSymbol(pr.data(), HIP_SYMBOL(fd_gemm16_probe), pr.size()*8));
      double cyc = 0, wall = 0; for (int b = 0; b < 256; ++b) { cyc += (double)(pr[8*b+1]-pr[8*b]); wall += (double)(pr[8*b+3]-pr[8*b+2]); }
      printf("ABL=%d K=2048: %.1f us; per workgroup main loop %.0f shader cycles in %.0f ticks of the constant 100 MHz counter -> %.3f GHz\n", abl, t, cyc/256, wall/256, cyc/wall*0.1);
    }
    return 0;
  }
  if (only == -2 || only == -1) {   // K sweep and ablations on the 6272 x 512 shape (TM 13, stride 196, 4 stages)
    for (int K : {128, 256, 512, 1024, 2048}) {
      const double fl = 2.0*6272*512*K;
      float t0 = run_new<13,4,0>(A,W,bias,out2,6272,512,K,196,20), t1 = run_new<13,4,1>(A,W,bias,out2,6272,512,K,196,20), t2 = run_new<13,4,2>(A,W,bias,out2,6272,512,K,196,20), t3 = run_new<13,4,3>(A,W,bias,out2,6272,512,K,196,20), t4 = run_new<13,4,4>(A,W,bias,out2,6272,512,K,196,20);
      float o = run_old<2,2,1,2>(A,W,bias,out,6272,512,K,20);
      printf("K=%4d  full %.1f us (%.0f TF) | no-dma %.1f (%.0f) | no-dma,no-frags %.1f (%.0f) | mfma only %.1f (%.0f) | full, no stores %.1f | old 64x128 %.1f (%.0f)\n", K, t0, fl/t0/1e6, t1, fl/t1/1e6, t2, fl/t2/1e6, t3, fl/t3/1e6, t4, o, fl/o/1e6);
    }
    fflush(stdout);
    if (only == -2) return 0;
  }
  int si = -1;
  for (auto s: shapes) { ++si; if (only >= 0 && si != only) continue;
    const double fl = 2.0*s.M*s.N*s.K;
    const int nt = (s.N+63)/64;
    float t_old[3] = { run_old<2,2,1,1>(A,W,bias,out,s.M,s.N,s.K,20), run_old<2,2,2,1>(A,W,bias,out,s.M,s.N,s.K,20), run_old<2,2,1,2>(A,W,bias,out,s.M,s.N,s.K,20) };
    run_old<2,2,1,1>(A,W,bias,out,s.M,s.N,s.K,1);
    printf("%dx%dx%d  old 64x64 %.1f us (%.0f TF)  128x64 %.1f (%.0f)  64x128 %.1f (%.0f)\n", s.M,s.N,s.K, t_old[0], fl/t_old[0]/1e6, t_old[1], fl/t_old[1]/1e6, t_old[2], fl/t_old[2]/1e6);
    // candidate strides: full tile, and the strides that make the grid r * 256 workgroups
    const int tms[3] = {13, 7, 4};
    for (int tm : tms) {
      std::vector<int> strides; strides.push_back(tm*16);
      for (int r = 1; r <= 16; ++r) { int mtiles = (256*r + nt - 1) / nt; int st = (s.M + mtiles - 1) / mtiles; if (st <= tm*16 && st * 100 >= tm*16 * (tm == 4 ? 75 : 86)) strides.push_back(st); }
      std::sort(strides.begin(), strides.end()); strides.erase(std::unique(strides.begin(), strides.end()), strides.end());
      for (int st : strides) {
        float t3 = 0, t4 = 0;
        if (tm == 13) { t3 = run_new<13,3>(A,W,bias,out2,s.M,s.N,s.K,st,20); t4 = run_new<13,4>(A,W,bias,out2,s.M,s.N,s.K,st,20); }
        if (tm == 7) { t3 = run_new<7,3>(A,W,bias,out2,s.M,s.N,s.K,st,20); t4 = run_new<7,4>(A,W,bias,out2,s.M,s.N,s.K,st,20); }
        if (tm == 4) { t3 = run_new<4,3>(A,W,bias,out2,s.M,s.N,s.K,st,20); t4 = run_new<4,4>(A,W,bias,out2,s.M,s.N,s.K,st,20); }
        const int mtl = (s.M + st - 1) / st;
        printf("   TM=%2d stride=%3d wgs=%5d (%.2f/CU)  S3 %.1f us (%.0f TF)  S4 %.1f us (%.0f TF)  maxrel %.2e\n", tm, st, mtl*nt, mtl*nt/256.0, t3, fl/t3/1e6, t4, fl/t4/1e6,
               maxdiff(out, out2, (size_t)s.M*s.N, ha, hb));
      }
    }
    fflush(stdout);
  }
  return 0;
}
