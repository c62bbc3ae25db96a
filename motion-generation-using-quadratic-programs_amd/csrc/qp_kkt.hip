// qp_kkt.hip — qpgpu_kkt_residuals / qpgpu_kkt_residuals_box: the KKT residuals of a batch of
// primal-dual pairs (x, u), eight doubles per QP (include/qpgpu.h).
//
// The definition fixes every sum's order (ascending index from +0.0, products rounded before they
// are added), so a sum is one lane's serial walk and the parallelism is across rows and columns:
//
//   one QP per group of S lanes of a wavefront (S = 8, 16, 32 or 64: the smallest that holds n, 64
//   beyond), 64 / S QPs per wave, four waves per workgroup, no workgroup barrier.  A matrix (G, CE,
//   CI) passes through a group-private LDS tile in coalesced pieces; lane r of the group then
//   walks row r of the tile (the row sums a, c, d and their magnitudes) and lane k walks column k
//   (the column sums e, s and theirs).  Accumulators live in the walking lane's registers.
//
//   rows sweep   tiles of S rows x 16 columns, row block outer, column chunk inner: a lane keeps
//                its row's two accumulators across the chunks.  With n <= S the one row block is
//                the whole column, so the same tile also completes the column sums of its 16
//                columns: CE and CI are read once.
//   cols sweep   n > 64 only (S = 64): tiles of 16 rows x 64 columns, column block outer, row chunk
//                inner: a lane keeps its column's two accumulators across the chunks.  CE and CI
//                are read a second time (G is not: it has no column sums); state stays O(1) per
//                lane for any n, p, m, which is what makes the kernel run-time sized without a
//                workspace.
//
// The running maxima (smax: a NaN is kept) and the minimum and the count over ui do not depend on
// the order of their operands — every operand is +0.0 or positive, resp. negative — so they are
// lane-local and meet in a shuffle tree over the group at the end.  q and l are ordered sums over
// i: the group's lane 0 adds the products of a row block from LDS, block after block.
//
// A group past the end of the batch recomputes the last QP and stores nothing; a QP masked by its
// status is computed like any other (its arrays exist) and stores NaN.  Every loop bound is the
// same in all lanes of a wave.
//
// The box kernel reads no CI: d_i, s_k and their magnitudes are the one or two non-zero terms of
// the dense sums (include/qpgpu.h), elementwise.
#include "qp_common.h"
#include "qp_kkt.h"

namespace qpk {

constexpr int kKktWaves = 4;  // wavefronts per workgroup
constexpr int kChunk = 16;    // the short side of a tile
constexpr int kTileElems = 64 * (kChunk + 1);  // rows sweep: S x (16 + 1) per group; cols sweep: 16 x (64 + 1)

struct KktLds {
  double tile[kTileElems];
  double vec[128];  // the walk's other factor: rv of the tile's columns (rows sweep), x of its rows (cols
                    // sweep); 16 per group, so 128 with S = 8
  double qs[64];   // x of the row block, then x_i * a_i for the group's ordered sum q
  double ls[64];   // g0_i * x_i for l
};

// A lane's group: its slices of the wave's LDS arrays (S slots each, max(S, 16) of vec; S * 17 of the tile).
struct KktGroup {
  double* tile;
  double* vec;
  double* qs;
  double* ls;
  int sl, S;  // lane within the group, lanes per group
};

__device__ __forceinline__ double kkt_ratio(double a, double b) { return b > 0.0 ? a / b : a; }
// the running maximum that keeps a NaN (include/qpgpu.h); commutative and associative on the
// values it meets here (+0.0, positive, NaN), so lanes may keep their own and merge at the end
__device__ __forceinline__ double kkt_smax(double acc, double v) {
  return acc != acc ? acc : ((v > acc || v != v) ? v : acc);
}

// What the sweeps leave in each lane; merged across the group at the end of the kernel.
struct KktAcc {
  double stat = 0.0, scale = 0.0, eq = 0.0, ineq = 0.0, comp = 0.0, umin = 0.0;
  int nnz = 0;
};

__device__ __forceinline__ void kkt_ineq_terms(KktAcc& acc, double s, double sa, double uk) {
  const double v = s < 0.0 ? kkt_ratio(-s, sa) : (s != s ? __builtin_nan("") : 0.0);
  acc.ineq = kkt_smax(acc.ineq, v);
  if (uk != 0.0) {
    acc.comp = kkt_smax(acc.comp, kkt_ratio(fabs(s), sa));
    acc.nnz++;
  }
  acc.umin = uk < acc.umin ? uk : acc.umin;
}

// Rows [i0, i0 + rows) x columns [k0, k0 + cw) of the row-major n x c matrix M of the group's QP
// (qb: the offset of its element 0; element e at + e * T) into tile[r * LD + cc], by the group's S
// lanes: lane-consecutive elements of the piece, so QP-major reads are whole contiguous runs.
// rows * cw <= 16 * S.
template <int T, int LD>
__device__ __forceinline__ void kkt_load_tile(double* tile, int sl, int S, const double* M, int64_t qb,
                                              int c, int i0, int rows, int k0, int cw) {
  const int total = rows * cw;
  const int dq = S / cw, dr = S % cw;
  int r = sl / cw, cc = sl % cw;
  double v[16];
  int at[16];
#pragma unroll
  for (int t = 0; t < 16; t++) {
    at[t] = -1;
    if (t * S < total) {  // wave-uniform
      if (r < rows) {
        v[t] = M[qb + ((int64_t)(i0 + r) * c + k0 + cc) * T];
        at[t] = r * LD + cc;
      }
      r += dq;
      cc += dr;
      if (cc >= cw) {
        cc -= cw;
        r++;
      }
    }
  }
#pragma unroll
  for (int t = 0; t < 16; t++)
    if (at[t] >= 0) tile[at[t]] = v[t];
}

// One matrix in the rows sweep: the row sums of rows [i0, i0 + rows) against rv (c values at
// rvp + k * T), into (s, sa) of group lane = row; with COLS (n <= S: the block is every row) also
// the column sums against x (g.qs) of every column, handed to fin(k, cs, csa) by the lane that
// walked column k.
template <int T, bool COLS, class Fin>
__device__ __forceinline__ void kkt_rows_sweep(const KktGroup& g, const double* M, int64_t qb, int c, int i0,
                                               int rows, const double* rvp, double& s, double& sa, Fin fin) {
  constexpr int LD = kChunk + 1;
  s = 0.0;
  sa = 0.0;
  for (int k0 = 0; k0 < c; k0 += kChunk) {
    const int cw = min(kChunk, c - k0);
    sg_sync();  // the previous tile's walks are done
    kkt_load_tile<T, LD>(g.tile, g.sl, g.S, M, qb, c, i0, rows, k0, cw);
    for (int cc = g.sl; cc < cw; cc += g.S) g.vec[cc] = rvp[(int64_t)(k0 + cc) * T];
    sg_sync();
    if (g.sl < rows) {
      for (int cc = 0; cc < cw; cc++) {
        const double v = g.tile[g.sl * LD + cc], w = g.vec[cc];
        const double pr = v * w, pa = fabs(v) * fabs(w);
        s = s + pr;
        sa = sa + pa;
      }
    }
    if constexpr (COLS) {
      for (int cc = g.sl; cc < cw; cc += g.S) {  // (two columns per lane with S = 8)
        double cs = 0.0, csa = 0.0;
        for (int r = 0; r < rows; r++) {
          const double v = g.tile[r * LD + cc], w = g.qs[r];
          const double pr = v * w, pa = fabs(v) * fabs(w);
          cs = cs + pr;
          csa = csa + pa;
        }
        fin(k0 + cc, cs, csa);
      }
    }
  }
}

// One matrix in the cols sweep (n > 64, the group is the wave): the column sums against x of
// every column.
template <int T, class Fin>
__device__ __forceinline__ void kkt_cols_sweep(const KktGroup& g, const double* M, int64_t qb, int n, int c,
                                               const double* xp, Fin fin) {
  constexpr int LD = 64 + 1;
  for (int k0 = 0; k0 < c; k0 += 64) {
    const int cw = min(64, c - k0);
    double cs = 0.0, csa = 0.0;
    for (int i0 = 0; i0 < n; i0 += kChunk) {
      const int rows = min(kChunk, n - i0);
      sg_sync();
      kkt_load_tile<T, LD>(g.tile, g.sl, 64, M, qb, c, i0, rows, k0, cw);
      if (g.sl < rows) g.vec[g.sl] = xp[(int64_t)(i0 + g.sl) * T];
      sg_sync();
      if (g.sl < cw) {
        for (int r = 0; r < rows; r++) {
          const double v = g.tile[r * LD + g.sl], w = g.vec[r];
          const double pr = v * w, pa = fabs(v) * fabs(w);
          cs = cs + pr;
          csa = csa + pa;
        }
      }
    }
    if (g.sl < cw) fin(k0 + g.sl, cs, csa);
  }
}

// over the S lanes of a group (S wave-uniform)
template <class F>
__device__ __forceinline__ double kkt_group_reduce(double v, int S, F f) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1)
    if (d < S) v = f(v, __shfl_xor(v, d, 64));
  return v;
}

template <int T, bool BOX>
__global__ void __launch_bounds__(64 * kKktWaves) kkt_kernel(KktArgs a) {
  __shared__ KktLds lds[kKktWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int S = a.group, sub = lane / S;
  const int64_t b_wave = a.qp0 + ((int64_t)blockIdx.x * kKktWaves + wave) * (64 / S);
  if (b_wave >= a.batch) return;  // whole waves: no workgroup barrier anywhere below
  const bool live = b_wave + sub < a.batch;
  const int64_t b = live ? b_wave + sub : a.batch - 1;
  KktLds& L = lds[wave];
  const KktGroup g = {L.tile + sub * S * (kChunk + 1), L.vec + sub * max(S, kChunk), L.qs + sub * S, L.ls + sub * S,
                      lane - sub * S, S};
  const int sl = g.sl;
  const int n = a.n, p = a.p, m = a.m;
  const bool masked = a.status && a.status[b] != QPGPU_QP_OK;
  const double* xp = a.x + qbase<T>(b, n);
  const double* g0p = a.g0 + qbase<T>(b, n);
  const double* up = (p + m > 0) ? a.u + qbase<T>(b, p + m) : a.x;  // (never read with p + m == 0)
  const double* uip = up + (int64_t)p * T;
  const int64_t qG = qbase<T>(b, n * n), qCE = qbase<T>(b, n * p), qCI = qbase<T>(b, n * m);
  const double* ce0p = p > 0 ? a.ce0 + qbase<T>(b, p) : nullptr;
  const double* ci0p = (!BOX && m > 0) ? a.ci0 + qbase<T>(b, m) : nullptr;

  KktAcc acc;
  const auto fin_eq = [&](int k, double cs, double csa) {
    const double c0 = ce0p[(int64_t)k * T];
    acc.eq = kkt_smax(acc.eq, kkt_ratio(fabs(cs + c0), csa + fabs(c0)));
  };
  const auto fin_ineq = [&](int k, double cs, double csa) {
    const double c0 = ci0p[(int64_t)k * T];
    kkt_ineq_terms(acc, cs + c0, csa + fabs(c0), uip[(int64_t)k * T]);
  };
  const auto no_fin = [](int, double, double) {};

  const bool one_block = n <= S;  // otherwise S = 64 and the group is the wave
  double q = 0.0, l = 0.0;        // group lane 0's
  for (int i0 = 0; i0 < n; i0 += S) {
    const int rows = min(S, n - i0);
    const bool row = sl < rows;
    const double xi = row ? xp[(int64_t)(i0 + sl) * T] : 0.0;
    const double gi = row ? g0p[(int64_t)(i0 + sl) * T] : 0.0;
    sg_sync();  // lane 0 has read the previous block's qs / ls
    g.qs[sl] = xi;  // x of this row block (the column walks' other factor), until a_i is known
    sg_sync();
    double s, sa, ts, t;
    // G: a_i, aa_i
    kkt_rows_sweep<T, false>(g, a.G, qG, n, i0, rows, xp, s, sa, no_fin);
    const double ai = s;
    t = s + gi;
    ts = sa + fabs(gi);
    // CE: c_i, ca_i (and e_k with n <= S)
    if (one_block)
      kkt_rows_sweep<T, true>(g, a.CE, qCE, p, i0, rows, up, s, sa, fin_eq);
    else
      kkt_rows_sweep<T, false>(g, a.CE, qCE, p, i0, rows, up, s, sa, no_fin);
    t = t - s;
    ts = ts + sa;
    // CI: d_i, da_i (and s_k with n <= S)
    if constexpr (BOX) {
      const double uu = row ? uip[(int64_t)(i0 + sl) * T] : 0.0;
      const double ul = row ? uip[(int64_t)(n + i0 + sl) * T] : 0.0;
      s = (0.0 - uu) + ul;
      sa = (0.0 + fabs(uu)) + fabs(ul);
    } else if (one_block) {
      kkt_rows_sweep<T, true>(g, a.CI, qCI, m, i0, rows, uip, s, sa, fin_ineq);
    } else {
      kkt_rows_sweep<T, false>(g, a.CI, qCI, m, i0, rows, uip, s, sa, no_fin);
    }
    t = t - s;
    ts = ts + sa;
    if (row) {
      acc.stat = kkt_smax(acc.stat, fabs(t));
      acc.scale = kkt_smax(acc.scale, ts);
    }
    sg_sync();  // every walk that reads x from qs is done
    g.qs[sl] = xi * ai;
    g.ls[sl] = gi * xi;
    sg_sync();
    if (sl == 0) {
      for (int r = 0; r < rows; r++) {
        q = q + g.qs[r];
        l = l + g.ls[r];
      }
    }
  }
  if (!one_block) {
    kkt_cols_sweep<T>(g, a.CE, qCE, n, p, xp, fin_eq);
    if constexpr (!BOX) kkt_cols_sweep<T>(g, a.CI, qCI, n, m, xp, fin_ineq);
  }
  if constexpr (BOX) {  // inequality k < n: the upper bound of x[k]; n + k: its lower bound
    const double* hip = a.hi + qbase<T>(b, n);
    const double* lop = a.lo + qbase<T>(b, n);
    for (int k = sl; k < n; k += S) {
      const double xk = xp[(int64_t)k * T], h = hip[(int64_t)k * T], lw = -lop[(int64_t)k * T];
      kkt_ineq_terms(acc, (0.0 - xk) + h, (0.0 + fabs(xk)) + fabs(h), uip[(int64_t)k * T]);
      kkt_ineq_terms(acc, (0.0 + xk) + lw, (0.0 + fabs(xk)) + fabs(lw), uip[(int64_t)(n + k) * T]);
    }
  }

  const auto mx = [](double x, double y) { return kkt_smax(x, y); };
  const double stat = kkt_group_reduce(acc.stat, S, mx), scale = kkt_group_reduce(acc.scale, S, mx);
  const double eq = kkt_group_reduce(acc.eq, S, mx), ineq = kkt_group_reduce(acc.ineq, S, mx);
  const double comp = kkt_group_reduce(acc.comp, S, mx);
  const double umin = kkt_group_reduce(acc.umin, S, [](double x, double y) { return y < x ? y : x; });
  int nnz = acc.nnz;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1)
    if (d < S) nnz += __shfl_xor(nnz, d, 64);
  if (sl == 0 && live) {
    double* rp = a.r + qbase<T>(b, QPGPU_KKT_NRES);
    const double nan = __builtin_nan("");
    rp[QPGPU_KKT_STAT * T] = masked ? nan : kkt_ratio(stat, scale);
    rp[QPGPU_KKT_STAT_SCALE * T] = masked ? nan : scale;
    rp[QPGPU_KKT_EQ * T] = masked ? nan : eq;
    rp[QPGPU_KKT_INEQ * T] = masked ? nan : ineq;
    rp[QPGPU_KKT_COMP * T] = masked ? nan : comp;
    rp[QPGPU_KKT_UMIN * T] = masked ? nan : umin;
    rp[QPGPU_KKT_OBJ * T] = masked ? nan : 0.5 * q + l;
    rp[QPGPU_KKT_NNZ * T] = masked ? nan : (double)nnz;
  }
}

}  // namespace qpk

// Enqueue the check of QPs [0, a->batch); box: a->hi is set and CI / ci0 are not read.
extern "C" hipError_t qpk_launch_kkt(const qpk::KktArgs* a, int tiled, hipStream_t stream) {
  qpk::KktArgs c = *a;
  c.group = a->n <= 8 ? 8 : a->n <= 16 ? 16 : a->n <= 32 ? 32 : 64;
  const int64_t per_wg = qpk::kKktWaves * (64 / c.group);  // QPs per workgroup
  const int64_t per = (int64_t)1 << 30;                     // workgroups per launch: the grid stays inside 32 bits
  for (int64_t w0 = 0; w0 * per_wg < a->batch; w0 += per) {
    c.qp0 = w0 * per_wg;
    const int64_t left = (a->batch - c.qp0 + per_wg - 1) / per_wg;
    const dim3 grid((unsigned)(left < per ? left : per)), block(64 * qpk::kKktWaves);
    if (a->hi) {
      if (tiled)
        hipLaunchKernelGGL((qpk::kkt_kernel<64, true>), grid, block, 0, stream, c);
      else
        hipLaunchKernelGGL((qpk::kkt_kernel<1, true>), grid, block, 0, stream, c);
    } else {
      if (tiled)
        hipLaunchKernelGGL((qpk::kkt_kernel<64, false>), grid, block, 0, stream, c);
      else
        hipLaunchKernelGGL((qpk::kkt_kernel<1, false>), grid, block, 0, stream, c);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
