// The shared kernels of gcn_mm.h, compiled once for the whole library: the generic tile GEMM k_gcn_mm with its
// launchers, the split-K weight gradient and the column sums.
#include "gcn_mm.h"

namespace gcm_mm {
namespace {

template <int NCT>
__global__ __launch_bounds__(256) void k_gcn_mm(MmArgs p) {
  __shared__ float sA[MB * (KT + 1)];        // [i][k]
  __shared__ float sB[KT * (32 * NCT + 1)];  // [k][j]
  const int b = blockIdx.z % p.batch, split = blockIdx.z / p.batch;
  const int i0 = blockIdx.x * MB, j0 = blockIdx.y * 32 * NCT;
  const TileLane t = tile_lane();
  const int kbeg = split * p.kchunk;
  const int kend = min(p.K, kbeg + p.kchunk);
  const float* Ab = p.A + (size_t)b * p.a_bs;
  const float* Bb = p.B + (size_t)b * p.b_bs;
  const float* ks = p.b_kscale ? p.b_kscale + (size_t)b * p.s_bs : nullptr;
  const bool a_rfast = p.a_is == 1 && p.a_ks != 1;  // coalesced order of the global reads
  const bool b_kfast = p.b_ks == 1 && p.b_js != 1;

  f32x16 acc[NCT];
  tile_zero(acc);
  tile_mma<NCT, false>(
      acc, t, sA, sB, i0, j0, p.M, p.N, kbeg, kend, a_rfast, b_kfast,
      [=](int gi, int gk) {
        return (p.a_diag && gi == gk) ? p.diag_val : Ab[(size_t)gi * p.a_is + (size_t)gk * p.a_ks];
      },
      [=](int gk, int gj) {
        float v = Bb[(size_t)gk * p.b_ks + (size_t)gj * p.b_js];
        if (ks) v *= ks[gk];
        return v;
      });

  float* Cb = p.C + (size_t)b * p.c_bs + (size_t)split * p.c_ss;
  const size_t so = (size_t)b * p.s_bs;
  tile_store(acc, t, i0, j0, p.M, p.N, [=](int j) {
    const float cs = p.c_cscale ? p.c_cscale[so + j] : 1.f;
    const float bias = p.c_bias ? p.c_bias[j] : 0.f;
    return [=](int i, float v) {
      const size_t off = (size_t)i * p.c_is + (size_t)j * p.c_js;
      if (p.C2) p.C2[(size_t)b * p.c_bs + off] = v;
      if (p.c_rscale) v *= p.c_rscale[so + i];
      v *= cs;
      if (p.c_radd) v += p.c_radd[so + i];
      v += bias;
      if (p.c_zero_diag && i == j) v = 0.f;
      Cb[off] = v;
    };
  });
}

// slabs[s, f] = sum of src[r, f] over the rows of block s
__global__ __launch_bounds__(256) void k_colsum_slabs(const float* __restrict__ src, int64_t R, int F,
                                                      float* __restrict__ slabs) {
  const int64_t r0 = (int64_t)blockIdx.x * COLSUM_ROWS;
  const int64_t r1 = min(R, r0 + COLSUM_ROWS);
  for (int f = threadIdx.x; f < F; f += 256) {
    float a = 0.f;
    for (int64_t r = r0; r < r1; ++r) a += src[(size_t)r * F + f];
    slabs[(size_t)blockIdx.x * F + f] = a;
  }
}

}  // namespace

int launch_mm(MmArgs p, int nsplit, hipStream_t s) {
  if (p.kchunk <= 0) p.kchunk = p.K;
  const int nct = nct_of(p.N);
  const int NC = 32 * nct;
  if ((int64_t)p.batch * nsplit > 65535) return GCM_EUNSUPPORTED;
  dim3 grid((p.M + MB - 1) / MB, (p.N + NC - 1) / NC, p.batch * nsplit);
  dispatch_nct(nct, [&](auto n) { hipLaunchKernelGGL(k_gcn_mm<n()>, grid, dim3(256), 0, s, p); });
  return gcm_launch_status();
}

int mm_xwt(const float* x, const float* w, const float* bias, float* y, int64_t R, int Fi, int Fo, hipStream_t s) {
  MmArgs p = mm_args();
  p.A = x, p.a_is = Fi, p.a_ks = 1;
  p.B = w, p.b_ks = 1, p.b_js = Fi;
  p.C = y, p.c_is = Fo, p.c_js = 1, p.c_bias = bias;
  p.M = (int)R, p.N = Fo, p.K = Fi;
  return launch_mm(p, 1, s);
}

int mm_gw(const float* g, const float* w, float* c, int64_t R, int Fi, int Fo, hipStream_t s, int batch, int64_t w_bs,
          int64_t c_bs) {
  MmArgs p = mm_args();
  p.A = g, p.a_is = Fo, p.a_ks = 1;
  p.B = w, p.b_bs = w_bs, p.b_ks = Fi, p.b_js = 1;
  p.C = c, p.c_bs = c_bs, p.c_is = Fi, p.c_js = 1;
  p.M = (int)R, p.N = Fi, p.K = Fo, p.batch = batch;
  return launch_mm(p, 1, s);
}

void wgrad_split(int64_t R, int* nsplit, int* kchunk) {
  int n = (int)std::min<int64_t>(256, (R + 511) / 512);
  n = std::max(n, 1);
  int64_t c = (R + n - 1) / n;
  c = (c + KT - 1) / KT * KT;
  *kchunk = (int)c;
  *nsplit = (int)((R + c - 1) / c);
}

void wgrad_split64(int64_t R, int* nsplit, int* kchunk) {
  int64_t c = std::max<int64_t>(64, (R + 511) / 512);
  c = (c + KT - 1) / KT * KT;
  *kchunk = (int)c;
  *nsplit = (int)((R + c - 1) / c);
}

int wgrad(const float* gy, const float* x, float* g, float* slabs, int64_t R, int Fi, int Fo, hipStream_t s,
          SplitPlan plan) {
  int nsplit, kchunk;
  plan(R, &nsplit, &kchunk);
  MmArgs p = mm_args();
  p.A = gy, p.a_is = 1, p.a_ks = Fo;
  p.B = x, p.b_ks = Fi, p.b_js = 1;
  p.C = slabs, p.c_is = Fi, p.c_js = 1, p.c_ss = (int64_t)Fo * Fi;
  p.M = Fo, p.N = Fi, p.K = (int)R, p.kchunk = kchunk;
  int rc = launch_mm(p, nsplit, s);
  if (rc) return rc;
  return gcm_sum_slabs(slabs, nsplit, Fo * Fi, g, s);
}

int colsum(const float* src, int64_t R, int F, float* out, float* slabs, hipStream_t s) {
  const int n = (int)colsum_slabs(R);
  hipLaunchKernelGGL(k_colsum_slabs, dim3(n), dim3(256), 0, s, src, R, F, slabs);
  const int rc = gcm_launch_status();
  return rc ? rc : gcm_sum_slabs(slabs, n, F, out, s);
}

int64_t colsum_slabs(int64_t R) { return (R + COLSUM_ROWS - 1) / COLSUM_ROWS; }

}  // namespace gcm_mm
