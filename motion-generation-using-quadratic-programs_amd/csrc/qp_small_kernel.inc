// qp_small_kernel.inc — the text of the subgroup kernel, included four times by qp_small.hip:
//   QP_SMALL_KERNEL = qp_small_kernel,      QP_SMALL_DUAL = false   (qpgpu_solve_batched)
//   QP_SMALL_KERNEL = qp_small_dual_kernel, QP_SMALL_DUAL = true    (qpgpu_solve_batched_dual)
//   QP_SMALL_KERNEL = qp_small_box_kernel,  QP_SMALL_BOX = true     (qpgpu_solve_batched_box)
//   QP_SMALL_KERNEL = qp_small_box_dual_kernel, both true           (qpgpu_solve_batched_box_dual)
//   QP_SMALL_KERNEL = qp_small_unit_kernel, QP_SMALL_UNIT = 1       (qpgpu_solve_batched_unit)
// UNIT (a preprocessor switch, so that the other four inclusions are the text they were): the
// Hessian is the identity and the setup is stated instead of computed — J = I, c1 = c2 = the sum of
// n ones, x0 = -g0, f0 from it; a.G is never read (DESIGN §3.10).
// The body stays inside the __global__ function, as it was before the dual mode existed: moved into
// a __device__ template that both kernels call, the S = 16 instantiations of the plain kernel
// allocated one VGPR fewer (421 -> 420, 490 -> 489), i.e. no longer the same code.
// DUAL (qpgpu_solve_batched_dual): r and u are carried over the whole active set — the equality
// phase runs the reference's update_r and its u[:iq] update, the loop's start at row 0 — and the
// multipliers leave through a.u / a.nact; x, f, status and the l1 passes are the same bits.
// BOX (qpgpu_solve_batched_box): the inequalities are lo <= x <= hi, i.e. CI = [-I, +I] and
// ci0 = [hi; -lo] never materialised.  A lane keeps the bound of each constraint it owns instead of
// a column of CI; the reference's sums over a column reduce to their one non-zero term added to the
// +0.0 the sum starts from (DESIGN §3.6).  a.CI / a.ci0 are not read.
// The two modes touch different statements, so both at once is the box kernel carrying r and u: the
// constraint index in A is the slot of u (upper bounds [p, p + n), lower [p + n, p + 2n)).
template <int S, int NM, int MM>
__global__ void __launch_bounds__(64) QP_SMALL_KERNEL(const QpArgs a) {
  constexpr bool DUAL = QP_SMALL_DUAL;
  constexpr bool BOX = QP_SMALL_BOX;
  using C = SmallCfg<S, NM, MM>;
  constexpr int RS = C::RS;
  constexpr int RPL = C::RPL;
  constexpr int CPL = C::CPL;
  __shared__ double lds_all[C::LDS_DOUBLES];

  const int lane = threadIdx.x;
  const int sg = lane / S;
  const int ls = lane - sg * S;
  const int64_t b = (int64_t)blockIdx.x * C::QPW + sg;
  if (b >= a.batch) return;  // the whole subgroup leaves together

  double* const Lq = lds_all + sg * C::REGION;
  double* const Rm = Lq + C::OFF_R;
  double* const Pm = Lq + C::OFF_P;
  double* const sb = Lq + C::OFF_S;
  double* const db = Lq + C::OFF_D;
  double* const zb = Lq + C::OFF_Z;
  double* const npb = Lq + C::OFF_NP;
  double* const xold = Lq + C::OFF_XOLD;
  double* const uold = Lq + C::OFF_UOLD;
  double* const aold = Lq + C::OFF_AOLD;

  const int n = a.n, p = a.p, m = a.m;
  const int T = a.tile;  // layout stride (include/qpgpu.h): 1 = QP-major, 64 = TILED64
  const double inf = dinf();
#if !QP_SMALL_UNIT
  const int64_t gbase = qbase_rt(b, n * n, T);
#endif

  // ---------------------------------------------------------------- loads
#if !QP_SMALL_UNIT
  {
    const double* Gb = a.G + gbase;
    for (int e = ls; e < n * n; e += S) {
      const int i = e / n;
      const int j = e - i * n;
      Pm[i * RS + j] = Gb[(int64_t)e * T];
    }
  }
#endif
  double CIr[BOX ? 1 : CPL][BOX ? 1 : NM];
  double ci0r[CPL];  // BOX: b = [hi; -lo] at this lane's constraints
  if constexpr (BOX) {
    const double* hib = a.hi + qbase_rt(b, n, T);
    const double* lob = a.lo + qbase_rt(b, n, T);
#pragma unroll
    for (int q = 0; q < CPL; q++) {
      const int c = ls + q * S;
      const bool up = c < n;
      const int v = up ? c : c - n;
      const double raw = c < m ? (up ? hib : lob)[(int64_t)v * T] : 0.0;
      ci0r[q] = up ? raw : -raw;
    }
    CIr[0][0] = 0.0;
  } else {
    const double* CIb = a.CI + qbase_rt(b, n * m, T);
    const double* ci0b = a.ci0 + qbase_rt(b, m, T);
#pragma unroll
    for (int q = 0; q < CPL; q++) {
      const int c = ls + q * S;
      const bool own = c < m;
#pragma unroll
      for (int j = 0; j < NM; j++) CIr[q][j] = (own && j < n) ? CIb[(int64_t)(j * m + c) * T] : 0.0;
      ci0r[q] = own ? ci0b[(int64_t)c * T] : 0.0;
    }
  }
  double g0v[NM];
#pragma unroll
  for (int i = 0; i < NM; i++) g0v[i] = (i < n) ? a.g0[qbase_rt(b, n, T) + (int64_t)i * T] : 0.0;
  sg_sync();

  int status = QPGPU_QP_OK;
  double fval = 0.0;
  int iter = 0;
  double xv[NM];
#pragma unroll
  for (int i = 0; i < NM; i++) xv[i] = 0.0;
  bool write_x = true;

#if QP_SMALL_UNIT
  // G = I stated: c1 = c2 = the ascending sum of n ones; nothing is loaded from G or factored
  double c1 = 0.0;
#pragma unroll
  for (int i = 0; i < NM; i++)
    if (i < n) c1 += 1.0;
  const bool chol_ok = true;
  const double bad_sum = 0.0;
#else
  // c1 = trace(G) before factorisation
  double c1 = 0.0;
#pragma unroll
  for (int i = 0; i < NM; i++)
    if (i < n) c1 += Pm[i * RS + i];

  // ---------------------------------------------------------------- Cholesky (in LDS)
  // cholesky_decomposition @.text+0x2df0: row-wise, descending-k sums, upper mirrored.
  bool chol_ok = true;
  double bad_sum = 0.0;
  for (int i = 0; i < n; i++) {
    double sum = Pm[i * RS + i];
    for (int k = i - 1; k >= 0; k--) sum -= Pm[i * RS + k] * Pm[i * RS + k];
    if (sum <= 0.0) {
      chol_ok = false;
      bad_sum = sum;
      break;
    }
    const double dg = sqrt(sum);
    for (int j = i + 1 + ls; j < n; j += S) {
      double s2 = Pm[i * RS + j];
      for (int k = i - 1; k >= 0; k--) s2 -= Pm[i * RS + k] * Pm[j * RS + k];
      Pm[j * RS + i] = s2 / dg;
    }
    if (ls == 0) Pm[i * RS + i] = dg;
    sg_sync();
    for (int k = i + 1 + ls; k < n; k += S) Pm[i * RS + k] = Pm[k * RS + i];
    sg_sync();
  }
  if (a.flags & QPGPU_FLAG_WRITE_FACTOR) {
    double* Gb = a.G + gbase;
    for (int e = ls; e < n * n; e += S) {
      const int i = e / n;
      const int j = e - i * n;
      Gb[(int64_t)e * T] = Pm[i * RS + j];
    }
  }
#endif  // QP_SMALL_UNIT

  if (!chol_ok) {
    status = QPGPU_QP_NOT_POSITIVE_DEFINITE;
    fval = bad_sum;
    write_x = false;
    if (a.x_eq && ls == 0) {
      a.f_eq[b] = fval;
      a.st_eq[b] = status;
    }
    if constexpr (DUAL) {  // no multipliers exist: the whole block +0.0
      double* ub = a.u + qbase_rt(b, p + m, T);
      for (int j = ls; j < p + m; j += S) ub[(int64_t)j * T] = 0.0;
      if (ls == 0 && a.nact) a.nact[b] = 0;
    }
  } else {
    // ---------------------------------------------------------------- J = L^{-T}
    double Jr[RPL][NM];
#if QP_SMALL_UNIT
    // J = I (+0.0 off the diagonal), x0 = -g0 (entries past n -0.0, as the dense setup's negation
    // of the +0.0 they start from)
#pragma unroll
    for (int q = 0; q < RPL; q++) {
      const int k = ls + q * S;
#pragma unroll
      for (int j = 0; j < NM; j++) Jr[q][j] = (k < n && j == k) ? 1.0 : 0.0;
    }
    const double c2 = c1;
#pragma unroll
    for (int i = 0; i < NM; i++) xv[i] = -g0v[i];
#else
#pragma unroll
    for (int q = 0; q < RPL; q++) {
      const int k = ls + q * S;
      double y[NM];
#pragma unroll
      for (int i = 0; i < NM; i++) {
        double v = 0.0;
        if (i < n) {
          v = (i == k) ? 1.0 : 0.0;
#pragma unroll
          for (int j = 0; j < i; j++) v -= Pm[i * RS + j] * y[j];
          v = v / Pm[i * RS + i];
        }
        y[i] = v;
      }
#pragma unroll
      for (int j = 0; j < NM; j++) Jr[q][j] = (k < n) ? y[j] : 0.0;
    }
    // c2 = trace(J), summed in row order
#pragma unroll
    for (int q = 0; q < RPL; q++) {
      const int k = ls + q * S;
      if (k < n) db[k] = sel<NM>(Jr[q], k);
    }
    sg_sync();
    double c2 = 0.0;
#pragma unroll
    for (int i = 0; i < NM; i++)
      if (i < n) c2 += db[i];

    // unconstrained minimiser: cholesky_solve (@.text+0x31a2), x = -G^{-1} g0
    {
      double y[NM];
#pragma unroll
      for (int i = 0; i < NM; i++) {
        double v = 0.0;
        if (i < n) {
          v = g0v[i];
#pragma unroll
          for (int j = 0; j < i; j++) v -= Pm[i * RS + j] * y[j];
          v = v / Pm[i * RS + i];
        }
        y[i] = v;
      }
#pragma unroll
      for (int i = NM - 1; i >= 0; i--) {
        if (i < n) {
          double v = y[i];
#pragma unroll
          for (int j = i + 1; j < NM; j++)
            if (j < n) v -= Pm[i * RS + j] * xv[j];
          xv[i] = v / Pm[i * RS + i];
        }
      }
#pragma unroll
      for (int i = 0; i < NM; i++) xv[i] = -xv[i];
    }
#endif  // QP_SMALL_UNIT
    fval = 0.0;
#pragma unroll
    for (int i = 0; i < NM; i++)
      if (i < n) fval += g0v[i] * xv[i];
    fval = 0.5 * fval;
    sg_sync();  // all reads of L done before P is reused

    // R = 0
    for (int e = ls; e < NM * RS; e += S) Rm[e] = 0.0;
    sg_sync();

    // ---------------------------------------------------------------- replicated state
    double dv[NM], zv[NM], npv[NM], uv[NM + 1], rv[NM];
    int Av[NM + 1];
#pragma unroll
    for (int i = 0; i < NM; i++) dv[i] = zv[i] = npv[i] = rv[i] = 0.0;
#pragma unroll
    for (int i = 0; i <= NM; i++) {
      uv[i] = 0.0;
      Av[i] = 0;
    }
    double npo[RPL];  // np at this lane's rows
    double R_norm = 1.0;
    int iq = 0;

    // compute_d: d[i] = sum_j J[j][i] np[j] (j ascending) via the LDS transpose P
    auto compute_d = [&]() {
#pragma unroll
      for (int q = 0; q < RPL; q++) {
        const int k = ls + q * S;
        if (k < n) {
#pragma unroll
          for (int c = 0; c < NM; c++)
            if (c < n) Pm[k * RS + c] = Jr[q][c] * npo[q];
        }
      }
      sg_sync();
#pragma unroll
      for (int q = 0; q < RPL; q++) {
        const int c = ls + q * S;
        if (c < n) {
          double s = 0.0;
#pragma unroll
          for (int j = 0; j < NM; j++)
            if (j < n) s += Pm[j * RS + c];
          db[c] = s;
        }
      }
      sg_sync();
#pragma unroll
      for (int i = 0; i < NM; i++) dv[i] = (i < n) ? db[i] : 0.0;
      sg_sync();
    };
    // update_z: z[i] = sum_{j>=iq} J[i][j] d[j] (row-local), then all-gathered
    auto update_z = [&]() {
#pragma unroll
      for (int q = 0; q < RPL; q++) {
        const int k = ls + q * S;
        double z = 0.0;
#pragma unroll
        for (int j = 0; j < NM; j++)
          if (j >= iq && j < n) z += Jr[q][j] * dv[j];
        if (k < n) zb[k] = z;
      }
      sg_sync();
#pragma unroll
      for (int i = 0; i < NM; i++) zv[i] = (i < n) ? zb[i] : 0.0;
      sg_sync();
    };
    // update_r: r = R[lo:iq, lo:iq]^{-1} d[lo:iq], back substitution (replicated).  Only the
    // inequality rows (lo = p) are computed: the equality constraints' rows feed only their
    // multipliers u[0..p), which nothing reads (t1, the dual step's drop and the rollback use the
    // inequalities' u; x and f never use u), and r[i] for i >= p does not depend on the rows
    // below.  For the same reason the equality phase runs none.
    auto update_r = [&](int lo) {
#pragma unroll
      for (int i = NM - 1; i >= 0; i--) {
        if (i >= lo && i < iq) {
          double s = 0.0;
#pragma unroll
          for (int j = i + 1; j < NM; j++)
            if (j < iq) s += Rm[i * RS + j] * rv[j];
          rv[i] = (dv[i] - s) / Rm[i * RS + i];
        }
      }
    };
    // add_constraint (@.text+0x21fd)
    auto add_constraint = [&]() -> bool {
      if (iq >= n) return false;  // reference UB (p > n); reported as dependent
#pragma unroll
      for (int j = NM - 1; j >= 1; j--) {
        if (j <= n - 1 && j >= iq + 1) {
          double cc = dv[j - 1], ss = dv[j];
          const double h = qp_distance(cc, ss);
          if (!(fabs(h) < kEps)) {
            dv[j] = 0.0;
            ss = ss / h;
            cc = cc / h;
            if (cc < 0.0) {
              cc = -cc;
              ss = -ss;
              dv[j - 1] = -h;
            } else {
              dv[j - 1] = h;
            }
            const double xny = ss / (1.0 + cc);
#pragma unroll
            for (int q = 0; q < RPL; q++) {
              const double t1 = Jr[q][j - 1], t2 = Jr[q][j];
              Jr[q][j - 1] = t1 * cc + t2 * ss;
              Jr[q][j] = xny * (t1 + Jr[q][j - 1]) - t2;
            }
          }
        }
      }
      iq++;
      if (ls == 0) {
#pragma unroll
        for (int i = 0; i < NM; i++)
          if (i < iq) Rm[i * RS + iq - 1] = dv[i];
      }
      sg_sync();
      const double dd = fabs(sel<NM>(dv, iq - 1));
      if (dd <= kEps * R_norm) return false;
      R_norm = (R_norm < dd) ? dd : R_norm;
      return true;
    };
    // delete_constraint (@.text+0x26a8)
    auto delete_constraint = [&](int l) {
      int qq = 0;
      bool found = false;
#pragma unroll
      for (int k = 0; k <= NM; k++)
        if (!found && k >= p && k < iq && Av[k] == l) {
          qq = k;
          found = true;
        }
#pragma unroll
      for (int i = 0; i < NM; i++)
        if (i >= qq && i < iq - 1) {
          Av[i] = Av[i + 1];
          uv[i] = uv[i + 1];
        }
      for (int j = ls; j < n; j += S)
        for (int i = qq; i < iq - 1; i++) Rm[j * RS + i] = Rm[j * RS + i + 1];
      {
        const int aiq = sel<NM + 1>(Av, iq);
        const double uiq = sel<NM + 1>(uv, iq);
        put<NM + 1>(Av, iq - 1, aiq);
        put<NM + 1>(uv, iq - 1, uiq);
        put<NM + 1>(Av, iq, 0);
        put<NM + 1>(uv, iq, 0.0);
      }
      for (int j = ls; j < iq; j += S) Rm[j * RS + iq - 1] = 0.0;
      iq--;
      sg_sync();
      if (iq == 0) return;
#pragma unroll
      for (int j = 0; j < NM - 1; j++) {
        if (j >= qq && j < iq) {
          double cc = Rm[j * RS + j], ss = Rm[(j + 1) * RS + j];
          const double h = qp_distance(cc, ss);
          if (!(fabs(h) < kEps)) {
            cc = cc / h;
            ss = ss / h;
            double nd;
            if (cc < 0.0) {
              nd = -h;
              cc = -cc;
              ss = -ss;
            } else {
              nd = h;
            }
            const double xny = ss / (1.0 + cc);
            for (int k = j + 1 + ls; k < iq; k += S) {
              const double t1 = Rm[j * RS + k], t2 = Rm[(j + 1) * RS + k];
              const double r1 = t1 * cc + t2 * ss;
              Rm[j * RS + k] = r1;
              Rm[(j + 1) * RS + k] = xny * (t1 + r1) - t2;
            }
            if (ls == 0) {
              Rm[(j + 1) * RS + j] = 0.0;
              Rm[j * RS + j] = nd;
            }
#pragma unroll
            for (int q = 0; q < RPL; q++) {
              const double t1 = Jr[q][j], t2 = Jr[q][j + 1];
              Jr[q][j] = t1 * cc + t2 * ss;
              Jr[q][j + 1] = xny * (Jr[q][j] + t1) - t2;
            }
          }
          sg_sync();
        }
      }
    };
    auto dot = [&](const double(&u_)[NM], const double(&v_)[NM]) -> double {
      double s = 0.0;
#pragma unroll
      for (int i = 0; i < NM; i++)
        if (i < n) s += u_[i] * v_[i];
      return s;
    };

    // BOX: constraint c bounds variable v = c mod n; sg a = -a for the upper bounds (c < n)
    [[maybe_unused]] auto box_sx = [&](int c) -> double {  // 0.0 + sg x[v]
      const bool up = c < n;
      const double xs = sel<NM>(xv, up ? c : c - n);
      return 0.0 + (up ? -xs : xs);
    };
    // BOX compute_d: d[i] = 0.0 + sg J[v][i], from the lane that holds row v of J
    [[maybe_unused]] auto compute_d_box = [&](int c) {
      const bool up = c < n;
      const int v = up ? c : c - n;
      if ((v % S) == ls) {
        const int qs = v / S;
#pragma unroll
        for (int i = 0; i < NM; i++)
          if (i < n) {
            double jv = opq(Jr[0][i]);
#pragma unroll
            for (int q = 1; q < RPL; q++) jv = (q == qs) ? opq(Jr[q][i]) : jv;
            db[i] = 0.0 + (up ? -jv : jv);
          }
      }
      sg_sync();
#pragma unroll
      for (int i = 0; i < NM; i++) dv[i] = (i < n) ? db[i] : 0.0;
      sg_sync();
    };

    // ---------------------------------------------------------------- equality phase
    bool done = false;
    for (int i = 0; i < p && !done; i++) {
      const double* CEb = a.CE + qbase_rt(b, n * p, T);
#pragma unroll
      for (int j = 0; j < NM; j++) npv[j] = (j < n) ? CEb[(int64_t)(j * p + i) * T] : 0.0;
#pragma unroll
      for (int q = 0; q < RPL; q++) {
        const int k = ls + q * S;
        npo[q] = (k < n) ? CEb[(int64_t)(k * p + i) * T] : 0.0;
      }
      compute_d();
      update_z();
      if constexpr (DUAL) update_r(0);  // the reference's: r for the u[:iq] update below
      double t2 = 0.0;
      const double zz = dot(zv, zv);
      const double znp = dot(zv, npv);
      if (fabs(zz) > kEps) t2 = (-dot(npv, xv) - a.ce0[qbase_rt(b, p, T) + (int64_t)i * T]) / znp;
#pragma unroll
      for (int k = 0; k < NM; k++) xv[k] += t2 * zv[k];
      put<NM + 1>(uv, iq, t2);
      if constexpr (DUAL) {
#pragma unroll
        for (int k = 0; k < NM; k++)
          if (k < iq) uv[k] -= t2 * rv[k];
      }
      fval += 0.5 * (t2 * t2) * znp;
      put<NM + 1>(Av, i, -i - 1);
      if (!add_constraint()) {
        status = QPGPU_QP_DEPENDENT;
        done = true;
      }
    }
    if (a.x_eq) {  // the m = 0 answer: an empty l1 scan returns right here
#pragma unroll
      for (int i = 0; i < NM; i++)
        if (i < n && (i % S) == ls) a.x_eq[qbase_rt(b, n, T) + (int64_t)i * T] = xv[i];
      if (ls == 0) {
        a.f_eq[b] = fval;
        a.st_eq[b] = status;
      }
    }

    // ---------------------------------------------------------------- active-set loop
    if (!done) {
      uint64_t act = 0;   // bit c set <=> iai[c] == -1
      uint64_t excl = 0;  // bit c set <=> iaexcl[c] == false
      int ip = 0, steps = 0;
      double ss = 0.0;
      bool need_scan = true, need_select = true;
      const int max_steps = a.max_steps;
      while (true) {
        if (need_scan) {  // ---- l1
          iter++;
#pragma unroll
          for (int k = 0; k < NM; k++)
            if (k >= p && k < iq) act |= 1ull << Av[k];
#pragma unroll
          for (int q = 0; q < CPL; q++) {
            const int c = ls + q * S;
            if (c < m) {
              double s = 0.0;
              if constexpr (BOX) {
                s = box_sx(c);
              } else {
#pragma unroll
                for (int j = 0; j < NM; j++)
                  if (j < n) s += CIr[q][j] * xv[j];
              }
              s += ci0r[q];
              sb[c] = s;
            }
          }
          sg_sync();
          excl = 0;
          ss = 0.0;
          ip = 0;
          double psi = 0.0;
#pragma unroll
          for (int i = 0; i < MM; i++)
            if (i < m) {
              const double si = sb[i];
              psi += (si < 0.0) ? si : 0.0;
            }
          if (fabs(psi) <= (double)m * kEps * c1 * c2 * 100.0) break;  // optimal
          if (ls == 0) {
#pragma unroll
            for (int i = 0; i < NM; i++) {
              if (i < iq) {
                uold[i] = uv[i];
                aold[i] = (double)Av[i];
              }
              xold[i] = xv[i];
            }
          }
          sg_sync();
        }
        if (need_select) {  // ---- l2 (ss deliberately not reset: reference quirk)
#pragma unroll
          for (int i = 0; i < MM; i++)
            if (i < m) {
              const double si = sb[i];
              const bool elig = !((act >> i) & 1ull) && !((excl >> i) & 1ull);
              if (si < ss && elig) {
                ss = si;
                ip = i;
              }
            }
          if (ss >= 0.0) break;  // optimal
          if constexpr (!BOX) {  // np gather (BOX forms no np in the loop); body left at its indentation
          if ((ip % S) == ls) {
            const int qs = ip / S;
#pragma unroll
            for (int j = 0; j < NM; j++)
              if (j < n) {
                double v = opq(CIr[0][j]);
#pragma unroll
                for (int q = 1; q < CPL; q++) v = (q == qs) ? opq(CIr[q][j]) : v;
                npb[j] = v;
              }
          }
          sg_sync();
#pragma unroll
          for (int i = 0; i < NM; i++) npv[i] = (i < n) ? npb[i] : 0.0;
#pragma unroll
          for (int q = 0; q < RPL; q++) {
            const int k = ls + q * S;
            npo[q] = (k < n) ? npb[k] : 0.0;
          }
          sg_sync();
          }
          put<NM + 1>(uv, iq, 0.0);
          put<NM + 1>(Av, iq, ip);
        }
        // ---- l2a
        if (max_steps > 0 && ++steps > max_steps) {
          status = QPGPU_QP_MAX_ITER;
          break;
        }
        if constexpr (BOX)
          compute_d_box(ip);
        else
          compute_d();
        update_z();
        update_r(DUAL ? 0 : p);
        int l = 0;
        double t1 = inf;
#pragma unroll
        for (int k = 0; k < NM; k++)
          if (k >= p && k < iq && rv[k] > 0.0) {
            const double q_ = uv[k] / rv[k];
            const bool take = q_ < t1;
            t1 = take ? q_ : t1;
            l = take ? opq(Av[k]) : l;
          }
        const double zz = dot(zv, zv);
        double znp;
        if constexpr (BOX) {
          const double zs = sel<NM>(zv, ip < n ? ip : ip - n);
          znp = 0.0 + (ip < n ? -zs : zs);
        } else {
          znp = dot(zv, npv);
        }
        double t2;
        if (fabs(zz) > kEps) {
          t2 = -sb[ip] / znp;
          if (t2 < 0) t2 = inf;  // Takano Akio patch
        } else {
          t2 = inf;
        }
        const double t = (t2 < t1) ? t2 : t1;
        if (t >= inf) {
          status = QPGPU_QP_INFEASIBLE;
          fval = inf;
          break;
        }
        if (t2 >= inf) {  // dual step only
#pragma unroll
          for (int k = 0; k < NM; k++)
            if ((DUAL || k >= p) && k < iq) uv[k] -= t * rv[k];
          put<NM + 1>(uv, iq, sel<NM + 1>(uv, iq) + t);
          act &= ~(1ull << l);
          delete_constraint(l);
          need_scan = need_select = false;
          continue;
        }
        // primal and dual step
#pragma unroll
        for (int k = 0; k < NM; k++) xv[k] += t * zv[k];
        fval += t * znp * (0.5 * t + sel<NM + 1>(uv, iq));
#pragma unroll
        for (int k = 0; k < NM; k++)
          if ((DUAL || k >= p) && k < iq) uv[k] -= t * rv[k];
        put<NM + 1>(uv, iq, sel<NM + 1>(uv, iq) + t);
        if (fabs(t - t2) < kEps) {  // full step
          if (!add_constraint()) {
            excl |= 1ull << ip;
            delete_constraint(ip);
            act = 0;
#pragma unroll
            for (int i = 0; i < NM; i++)
              if (i >= p && i < iq) {
                Av[i] = (int)aold[i];
                uv[i] = uold[i];
                act |= 1ull << Av[i];
              }
#pragma unroll
            for (int i = 0; i < NM; i++) xv[i] = xold[i];
            need_scan = false;
            need_select = true;
          } else {
            act |= 1ull << ip;
            need_scan = need_select = true;
          }
          continue;
        }
        // partial step: drop l, refresh s[ip]
        act &= ~(1ull << l);
        delete_constraint(l);
        if ((ip % S) == ls) {
          const int qs = ip / S;
          double s = 0.0;
          if constexpr (BOX) {
            s = box_sx(ip);
          } else {
#pragma unroll
            for (int j = 0; j < NM; j++)
              if (j < n) {
                double v = opq(CIr[0][j]);
#pragma unroll
                for (int q = 1; q < CPL; q++) v = (q == qs) ? opq(CIr[q][j]) : v;
                s += v * xv[j];
              }
          }
          double c0 = opq(ci0r[0]);
#pragma unroll
          for (int q = 1; q < CPL; q++) c0 = (q == qs) ? opq(ci0r[q]) : c0;
          sb[ip] = s + c0;
        }
        sg_sync();
        need_scan = need_select = false;
      }
    }
    if constexpr (DUAL) {
      // u dense, like x: equality j's multiplier is u[j] (A[j] = -j-1: equalities never move);
      // inequality A[k]'s is u[k] (k in [p, iq)), scattered through the s array in LDS so that
      // the stores are one per lane and slot; every other slot and every non-OK QP +0.0
      const bool okq = status == QPGPU_QP_OK;
      double* ub = a.u + qbase_rt(b, p + m, T);
      sg_sync();  // every lane's reads of s are over
      for (int i = ls; i < m; i += S) sb[i] = 0.0;
      sg_sync();
      if (ls == 0 && okq) {
#pragma unroll
        for (int k = 0; k < NM; k++)
          if (k >= p && k < iq) sb[Av[k]] = uv[k];
      }
      sg_sync();
      for (int j = ls; j < p; j += S) ub[(int64_t)j * T] = (okq && j <= NM) ? sel<NM + 1>(uv, j) : 0.0;
      for (int i = ls; i < m; i += S) ub[(int64_t)(p + i) * T] = sb[i];
      if (ls == 0 && a.nact) a.nact[b] = okq ? iq - p : 0;
    }
  }

  // ---------------------------------------------------------------- outputs
  if (write_x) {
#pragma unroll
    for (int i = 0; i < NM; i++)
      if (i < n && (i % S) == ls) a.x[qbase_rt(b, n, T) + (int64_t)i * T] = xv[i];
  }
  if (ls == 0) {
    a.f[b] = fval;
    a.status[b] = status;
    if (a.iters) a.iters[b] = iter;
  }
}

