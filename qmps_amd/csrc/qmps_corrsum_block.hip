// qmps_corrsum_block.hip - the correlator-sum kernels of the large bond dimensions (formulas: qmps_corrsum.hip; the elimination,
// the tiles and the source interface: qmps_corrsum_core.h), one instantiation per source:
//   D = 8   one workgroup of 256 threads per item, the 64 x (64 + n_ops) matrix in LDS, column-major (lanes read consecutive rows:
//           no bank conflict; the pivot row is a broadcast read); wave w owns the columns = w mod 4
//   D = 16  one workgroup of 256 threads (thread = row) per item, the 256 x (256 + n_ops) matrix column-major in a global workspace
//           of one slab per workgroup; a fixed grid of at most kMaxSlabs workgroups strides over the items (workspace <= 256 MiB)
#include "qmps_corrsum_internal.h"
#include "qmps_corrsum_one_site.h"
#include "qmps_corrsum_two_site.h"

namespace qmps {

namespace {

template <class Src>
__global__ __launch_bounds__(256) void corrsum_lds_kernel(CorrSumArgs p) {
  constexpr int D = 8, N = 64, NC = N + kMaxObservableOps;
  __shared__ double2 sW[NC][N];          // column-major: sW[column][row]
  __shared__ BlockTiles<D> S;
  __shared__ double2 sPiv[NC];
  const int tid = threadIdx.x, row = tid % N, part = tid / N, i = row / D, j = row % D;
  const int64_t it = blockIdx.x;
  const int64_t b = it / p.n_z;
  const int jz = (int)(it % p.n_z);
  const int m = p.n_ops, nc = N + m;
  const double2* O = (const double2*)p.ops;
  const double2 z = ((const double2*)p.z)[jz];
  double2 inv, tr[2][2];
  block_build<D>(S, (const double2*)p.A + b * (2 * N), (const double2*)p.r + b * N, tid, inv, tr);
  Src::template block_finish<D>(S, p, b, jz == 0, O, m, inv, tr, tid);
  const double2 rij = S.r[i][j], rs = cmul(rij, inv);
  for (int c = part; c < N; c += 4) sW[c][row] = matrix_entry<D>(S, z, rs, i, j, c / D, c % D);
  if (part < m) sW[N + part][row] = Src::template block_rhs<D>(S, O, inv, tr, rij, part, row);
  __syncthreads();

  bool used = false, bad = false;
  int colof = 0;
  for (int k = 0; k < N; ++k) {
    const double2 f = sW[k][row];
    double v = used ? -1.0 : pivot_size(f);
    int pr = row;
    wave_argmax(v, pr);                  // every wave searches the whole column: the same answer in all four
    bad = bad || !pivot_usable(v);
    const bool is = pr == row;
    const double2 ip = crecip(sW[k][pr]);
    for (int c = k + 1 + tid; c < nc; c += 256) sPiv[c] = cmul(sW[c][pr], ip);
    __syncthreads();
    for (int c = k + 1 + part; c < nc; c += 4) {
      const double2 pv = sPiv[c];
      double2 x = sW[c][row];
      cfms(f, pv, x);
      sW[c][row] = csel(is, pv, x);
    }
    used = used || is;
    colof = is ? k : colof;
    __syncthreads();
  }

  // wave c sums column N + c against every L_a
  if (part < m) {
    const double2 x = sW[N + part][row];
    const double2 scale = Src::readout_scale(z, inv);
    for (int a = 0; a < m; ++a) {
      const double2 w = cmul(S.lv[a][colof], x);
      const double2 s = make_double2(wave_sum(w.x), wave_sum(w.y));
      if (row == 0) ((double2*)p.G)[(it * m + a) * m + part] = bad ? cnan() : cmul(scale, s);
    }
  }
}

constexpr int kSlabColumns = 256 + kMaxObservableOps;
constexpr size_t kSlabBytes = (size_t)kSlabColumns * 256 * sizeof(double2);

template <class Src>
__global__ __launch_bounds__(256) void corrsum_global_kernel(CorrSumArgs p) {
  constexpr int D = 16, N = 256;
  __shared__ BlockTiles<D> S;
  __shared__ double2 sPiv[kSlabColumns];
  __shared__ double sRedV[4];
  __shared__ int sRedI[4];
  __shared__ double sSum[4][2 * kMaxObservableOps * kMaxObservableOps];
  const int tid = threadIdx.x, row = tid, i = row / D, j = row % D, wave = tid >> 6;
  const int m = p.n_ops, nc = N + m;
  const double2* O = (const double2*)p.ops;
  double2* Wg = (double2*)((char*)p.work + (size_t)blockIdx.x * kSlabBytes);      // column-major: Wg[column * N + row]
  const int64_t items = p.B * p.n_z;
  for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
    const int64_t b = it / p.n_z;
    const int jz = (int)(it % p.n_z);
    const double2 z = ((const double2*)p.z)[jz];
    double2 inv, tr[2][2];
    block_build<D>(S, (const double2*)p.A + b * (2 * N), (const double2*)p.r + b * N, tid, inv, tr);
    Src::template block_finish<D>(S, p, b, jz == 0, O, m, inv, tr, tid);
    const double2 rij = S.r[i][j], rs = cmul(rij, inv);
    for (int c = 0; c < N; ++c) Wg[c * N + row] = matrix_entry<D>(S, z, rs, i, j, c / D, c % D);
    for (int c = 0; c < m; ++c) Wg[(N + c) * N + row] = Src::template block_rhs<D>(S, O, inv, tr, rij, c, row);
    __syncthreads();

    bool used = false, bad = false;
    int colof = 0;
    for (int k = 0; k < N; ++k) {
      const double2 f = Wg[k * N + row];
      double v = used ? -1.0 : pivot_size(f);
      int pr = row;
      wave_argmax(v, pr);
      if ((tid & 63) == 0) {
        sRedV[wave] = v;
        sRedI[wave] = pr;
      }
      __syncthreads();
      v = sRedV[0];
      pr = sRedI[0];
#pragma unroll
      for (int w = 1; w < 4; ++w) {
        const double ov = sRedV[w];
        const int oi = sRedI[w];
        if (ov > v) {                    // rows of a later wave are higher: a tie keeps the earlier one
          v = ov;
          pr = oi;
        }
      }
      bad = bad || !pivot_usable(v);
      const bool is = pr == row;
      const double2 ip = crecip(Wg[k * N + pr]);
      for (int c = k + 1 + tid; c < nc; c += 256) sPiv[c] = cmul(Wg[c * N + pr], ip);
      __syncthreads();
#pragma unroll 4
      for (int c = k + 1; c < nc; ++c) {
        const double2 pv = sPiv[c];
        double2 x = Wg[c * N + row];
        cfms(f, pv, x);
        Wg[c * N + row] = csel(is, pv, x);
      }
      used = used || is;
      colof = is ? k : colof;
      __syncthreads();
    }

    for (int c = 0; c < m; ++c) {
      const double2 x = Wg[(N + c) * N + row];
      for (int a = 0; a < m; ++a) {
        const double2 w = cmul(S.lv[a][colof], x);
        const double sx = wave_sum(w.x), sy = wave_sum(w.y);
        if ((tid & 63) == 0) {
          sSum[wave][2 * (a * m + c)] = sx;
          sSum[wave][2 * (a * m + c) + 1] = sy;
        }
      }
    }
    __syncthreads();
    if (tid < m * m) {
      double2 s = make_double2(0.0, 0.0);
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        s.x += sSum[w][2 * tid];
        s.y += sSum[w][2 * tid + 1];
      }
      ((double2*)p.G)[it * (m * m) + tid] = bad ? cnan() : cmul(Src::readout_scale(z, inv), s);
    }
    __syncthreads();                     // the tiles and the slab are rebuilt for the next item
  }
}

}  // namespace

template <class Src>
void launch_block(int D, const CorrSumArgs& a, int64_t items, hipStream_t st) {
  if (D == 8) hipLaunchKernelGGL(corrsum_lds_kernel<Src>, dim3((unsigned)items), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(corrsum_global_kernel<Src>, dim3((unsigned)(items < a.n_slabs ? items : a.n_slabs)), dim3(256), 0, st, a);
}
template void launch_block<OneSiteSource>(int, const CorrSumArgs&, int64_t, hipStream_t);
template void launch_block<TwoSiteSource>(int, const CorrSumArgs&, int64_t, hipStream_t);

int64_t correlator_sums_slabs(int D, int64_t items) {
  if (D != 16) return 0;
  return items < kCorrSumMaxSlabs ? items : kCorrSumMaxSlabs;
}
size_t correlator_sums_slab_bytes() { return kSlabBytes; }

}  // namespace qmps
