// qmps_block_rdm.hip - reduced density matrices of n = 1 .. 4 contiguous sites of the resident states (qmps_block_entanglement):
//   B_t = A_t1 A_t2 .. A_tn,  t = sum_k t_k 2^(n-k)  (t1 the left site, most significant),   rho[t][s] = tr(B_t r B_s^+) / tr r,
// in ONE launch whatever n is.  A and r are fetched once per evaluation.  The products are built by doubling,
//   B^(k+1)[2t + s] = B^(k)[t] A_s   (B^(1) = A),
// in LDS up to level n - 1; the last level and M_t = B_t r = B^(n-1)[t >> 1] (A_(t & 1) r) go straight into registers, so a level costs what
// it holds and n = 1 builds nothing.  rho is the Gram matrix rho[t][s] = sum_ij M_t[i][j] conj(B_s[i][j]), a (2^n x D^2)(D^2 x 2^n)
// product: the last level is transposed through LDS ([t][ij], a quarter of the ij at a time at D = 8, 16, where LDS would not hold
// it whole) and thread g of the workgroup sums element g of the workgroup's rho, which is one contiguous run of global memory.
//   One thread per matrix element (i, j): D = 2, 4, 8 workgroups of one wave with 16 / 4 / 1 evaluations, D = 16 four waves with one.
// Every loop has a trip count fixed by D and n; there are no atomics, counters or waits between workgroups.  Dynamic LDS, sized by n.
// An evaluation whose tr r is zero or not finite is NaN throughout (crecip); a non-finite element of r reaches every element of rho.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qmps_kernels.h"
#include "qmps_complex.h"
#include "qmps_observable.h"

namespace qmps {

namespace {

// LDS of one evaluation, in double2: A (2 matrices), A r (2), r (1), then one region that holds the levels 2 .. n - 1 of the doubling
// (2^(n-1) matrices when n >= 3) and after them the two operands of the Gram product, 2^n rows of (D^2 / NCH + 1) each
template <int D, int NCH>
__host__ __device__ constexpr int block_rdm_region(int n) {
  const int levels = n >= 3 ? (1 << (n - 1)) * D * (D + 1) : 0, gram = 2 * (1 << n) * (D * D / NCH + 1);
  return levels > gram ? levels : gram;
}
template <int D, int NCH>
__host__ __device__ constexpr int block_rdm_eval(int n) {
  return 5 * D * (D + 1) + block_rdm_region<D, NCH>(n);
}

template <int D, int NCH>
__global__ __launch_bounds__(D* D < 64 ? 64 : D * D) void block_rdm_kernel(BlockRdmArgs p) {
  constexpr int N = D * D, NT = N < 64 ? 64 : N, EV = NT / N, P = D + 1, MS = D * P, CH = N / NCH, CS = CH + 1;
  constexpr int ACC = NCH == 1 ? 1 : (256 + NT - 1) / NT;       // elements of rho per thread where the Gram product runs in parts
  static_assert(NCH == 1 || EV == 1, "the Gram product runs in parts only where a workgroup holds one evaluation");
  extern __shared__ double2 smem[];
  const int n = p.n_sites, T = 1 << n, TT = T * T, ES = block_rdm_eval<D, NCH>(n);
  const int tid = threadIdx.x, e = tid / N, tl = tid % N, i = tl / D, j = tl % D;
  const int64_t b0 = (int64_t)blockIdx.x * EV;
  const int nb = p.B - b0 < EV ? (int)(p.B - b0) : EV;
  // threads past the batch work on a copy of the last evaluation (in their own LDS) and store nothing
  const int64_t b = e < nb ? b0 + e : p.B - 1;
  double2* sInv = smem;                                          // [EV]: 1 / tr r
  double2* mine = smem + EV + e * ES;
  double2 *sA = mine, *sAr = mine + 2 * MS, *sR = mine + 4 * MS, *sU = mine + 5 * MS;
  {
    const double2* a = (const double2*)p.A + b * (2 * N);
    sA[i * P + j] = a[tl];
    sA[MS + i * P + j] = a[N + tl];
    sR[i * P + j] = ((const double2*)p.r)[b * N + tl];
  }
  __syncthreads();
  if (tl == 0) {
    double2 tr = make_double2(0.0, 0.0);
#pragma unroll
    for (int l = 0; l < D; ++l) {
      tr.x += sR[l * P + l].x;
      tr.y += sR[l * P + l].y;
    }
    sInv[e] = crecip(tr);
  }
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    double2 v = make_double2(0.0, 0.0);
#pragma unroll
    for (int l = 0; l < D; ++l) cfma(sA[s * MS + i * P + l], sR[l * P + j], v);
    sAr[s * MS + i * P + j] = v;
  }
  __syncthreads();

  // levels 2 .. n - 1 (level 1 is A where it lies); a level is computed from its predecessor into registers and then overwrites it
  const double2* lev = sA;
  for (int k = 1; k + 1 < n; ++k) {
    const int cnt = 1 << k;
    double2 nx[8];
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (t < cnt) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          double2 v = make_double2(0.0, 0.0);
#pragma unroll
          for (int l = 0; l < D; ++l) cfma(lev[t * MS + i * P + l], sA[s * MS + l * P + j], v);
          nx[2 * t + s] = v;
        }
      }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 8; ++t)
      if (t < 2 * cnt) sU[t * MS + i * P + j] = nx[t];
    __syncthreads();
    lev = sU;
  }

  // the last level: element (i, j) of B_t and of M_t = B_t r for every t
  double2 Bf[16], Mf[16];
  if (n == 1) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      Bf[s] = sA[s * MS + i * P + j];
      Mf[s] = sAr[s * MS + i * P + j];
    }
  } else {
    const int half = T >> 1;
#pragma unroll
    for (int t = 0; t < 8; ++t)
      if (t < half) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          double2 vb = make_double2(0.0, 0.0), vm = make_double2(0.0, 0.0);
#pragma unroll
          for (int l = 0; l < D; ++l) {
            const double2 x = lev[t * MS + i * P + l];
            cfma(x, sA[s * MS + l * P + j], vb);
            cfma(x, sAr[s * MS + l * P + j], vm);
          }
          Bf[2 * t + s] = vb;
          Mf[2 * t + s] = vm;
        }
      }
  }

  // the Gram product, NCH parts of CH of the ij: the owners of a part lay their B_t and M_t down as rows [t][ij] (over the levels,
  // which nobody reads any more after the barrier), then thread g sums its element(s) of rho over the part
  double2* sBt = sU;
  double2* sMt = sU + T * CS;
  double2 acc[ACC];
#pragma unroll
  for (int m = 0; m < ACC; ++m) acc[m] = make_double2(0.0, 0.0);
  double2* out = (double2*)p.rho + b0 * TT;
#pragma unroll 1
  for (int c = 0; c < NCH; ++c) {
    __syncthreads();
    if (tl / CH == c) {
      const int cc = tl % CH;
#pragma unroll
      for (int t = 0; t < 16; ++t)
        if (t < T) {
          sBt[t * CS + cc] = Bf[t];
          sMt[t * CS + cc] = Mf[t];
        }
    }
    __syncthreads();
    if constexpr (NCH == 1) {
      // the workgroup's evaluations are one run of nb * 4^n elements: thread g takes the elements g, g + 64, ..
      const int total = nb * TT;
      for (int g = tid; g < total; g += NT) {
        const int ge = g >> (2 * n), idx = g & (TT - 1), t = idx >> n, s = idx & (T - 1);
        const double2* uB = smem + EV + ge * ES + 5 * MS;
        const double2* uM = uB + T * CS;
        double2 v = make_double2(0.0, 0.0);
#pragma unroll
        for (int cc = 0; cc < CH; ++cc) cfma_conj(uM[t * CS + cc], uB[s * CS + cc], v);
        out[g] = cmul(v, sInv[ge]);
      }
    } else {
#pragma unroll
      for (int m = 0; m < ACC; ++m) {
        const int g = tid + m * NT;
        if (g < TT) {
          const int t = g >> n, s = g & (T - 1);
          double2 v = acc[m];
#pragma unroll 8
          for (int cc = 0; cc < CH; ++cc) cfma_conj(sMt[t * CS + cc], sBt[s * CS + cc], v);
          acc[m] = v;
        }
      }
    }
  }
  if constexpr (NCH > 1) {
    const double2 inv = sInv[0];
#pragma unroll
    for (int m = 0; m < ACC; ++m) {
      const int g = tid + m * NT;
      if (g < TT) out[g] = cmul(acc[m], inv);
    }
  }
}

template <int D, int NCH>
hipError_t launch(const BlockRdmArgs& a, hipStream_t st) {
  constexpr int N = D * D, NT = N < 64 ? 64 : N, EV = NT / N;
  const size_t lds = (size_t)(EV + EV * block_rdm_eval<D, NCH>(a.n_sites)) * sizeof(double2);
  hipLaunchKernelGGL((block_rdm_kernel<D, NCH>), dim3((unsigned)((a.B + EV - 1) / EV)), dim3(NT), lds, st, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_block_rdm(int D, const BlockRdmArgs& a, hipStream_t st) {
  if (a.B <= 0) return hipSuccess;
  if (!a.A || !a.r || !a.rho || a.n_sites < 1 || a.n_sites > kMaxBlockSites) return hipErrorInvalidValue;
  switch (D) {
    case 2: return launch<2, 1>(a, st);
    case 4: return launch<4, 1>(a, st);
    case 8: return launch<8, 4>(a, st);
    case 16: return launch<16, 4>(a, st);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace qmps
