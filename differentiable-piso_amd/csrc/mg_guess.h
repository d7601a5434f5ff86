// Starting the multigrid PCG of mg.hip from a GUESS x0 (opt-in: piso_mg_pcg_solve*_guess_*; tests/mg_reference_guess.py is the numpy twin).
// Three small launches take the place of mg_init when a guess is given:
//   mg_guess_residual  r_g = b' - L x0~ on the present cells (x0~ = x0 there, 0 elsewhere: garbage on absent cells is never read into a sum),
//                      with the expression of mg_residual; fixed-order per-block partial maxima of |r_g| and |b'|, NaN propagating.  It
//                      reads x0 and writes r only: x0 may be x_out itself.
//   mg_guess_pick      one workgroup: m_g = max|r_g|, m_b = max|b'| from the partials in index order.  The guess is ACCEPTED iff
//                      m_g < m_b (strict; false for a NaN or Inf in r_g, and for x0 = 0, whose residual IS b'); otherwise
//                      MG_FLAG_GUESS_REJECTED goes into MgState.flags, which the host's regular look copies anyway.  Accepted and
//                      m_g < accuracy: done with 0 iterations - every kernel queued after it returns at once.
//   mg_guess_apply     accepted: x = x0~ (r_g stays where it is; float32 cycle: fl32(r_g) beside it).  Rejected: x = 0, r = b' with the
//                      expressions of mg_init - from here on the solve is the one without a guess, bit for bit.
// The guard exists because a previous time step's pressure increment is a WORSE start than zero in a start-up transient (its residual
// exceeds the right-hand side; DESIGN.md 3.7 has the counts): such a guess becomes a plain solve, never a failure.
// Constant mode: r_g is mean-free whatever the mean of x0 (the columns of L sum to zero), and the end of the solve replaces the mean of x.
#pragma once

namespace piso {

enum { MG_FLAG_GUESS_REJECTED = 16 };

__global__ __launch_bounds__(kBlock) void mg_guess_residual(Lv L, const double* __restrict__ b, const double* __restrict__ x0, double* __restrict__ r,
                                                            const double* scal, double* part_g, double* part_b, const MgState* st) {
  if (st->done) return;                                                  // (a prepared solve on a buffer that is no hierarchy of this grid)
  __shared__ double smem[16];
  const double mean = scal[SC_MEAN_B];
  double mg = 0, mb = 0;
  const Walk w = grid_walk();
  for (int c = w.begin; c < L.n; c += w.step) {
    double rv = 0.0;
    if (L.dinv[c] != 0) {
      const int j = c / L.nx, i = c - j * L.nx;
      const Nb q = neighbours(c, i, j, L.nx, L.ny);
      const double xs = L.dinv[q.s] != 0 ? x0[q.s] : 0.0, xw = L.dinv[q.w] != 0 ? x0[q.w] : 0.0;
      const double xe = L.dinv[q.e] != 0 ? x0[q.e] : 0.0, xn = L.dinv[q.n] != 0 ? x0[q.n] : 0.0;
      const double bp = b[c] - mean;
      rv = bp - stencil(L, c, xs, xw, x0[c], xe, xn);
      mb = nanmax(mb, fabs(bp));
    }
    r[c] = rv;
    mg = nanmax(mg, fabs(rv));
  }
  mg = mg_block_max_nan(mg, smem);
  mb = mg_block_max_nan(mb, smem);
  if (threadIdx.x == 0) { part_g[blockIdx.x] = mg; part_b[blockIdx.x] = mb; }
}

__global__ __launch_bounds__(kBlock) void mg_guess_pick(const double* part_g, const double* part_b, int count, float accuracy, MgState* st) {
  if (st->done) return;
  __shared__ double smem[16];
  double mg = 0, mb = 0;
  for (int k = threadIdx.x; k < count; k += blockDim.x) { mg = nanmax(mg, part_g[k]); mb = nanmax(mb, part_b[k]); }
  mg = mg_block_max_nan(mg, smem);
  mb = mg_block_max_nan(mb, smem);
  if (threadIdx.x == 0) {
    if (!(mg < mb)) st->flags |= MG_FLAG_GUESS_REJECTED;                 // (NaN, Inf, and a residual no smaller than the right-hand side)
    else if (mg < (double)accuracy) { st->iterations = 0; st->done = 1; }
  }
}

// (x0 may be x; no __restrict__ on the two: a thread reads its own cell of x0 and then writes that cell of x)
// R: the type of the cycle's values; under the float32 cycle rc = fl32(r) is written beside r
template <typename R>
__global__ __launch_bounds__(kBlock) void mg_guess_apply(Lv L, const double* __restrict__ b, const double* x0, double* x, double* __restrict__ r, const double* scal,
                                                         const MgState* st, R* __restrict__ rc) {
  constexpr bool R32 = std::is_same<R, float>::value;
  const bool rejected = (st->flags & MG_FLAG_GUESS_REJECTED) != 0;
  const double mean = scal[SC_MEAN_B];
  const Walk w = grid_walk();
  for (int c = w.begin; c < L.n; c += w.step) {
    const bool present = L.dinv[c] != 0;
    if (rejected) {
      x[c] = 0;
      const double rv = present ? b[c] - mean : 0.0;
      r[c] = rv;
      if constexpr (R32) rc[c] = (float)rv;
    } else {
      x[c] = present ? x0[c] : 0.0;
      if constexpr (R32) rc[c] = (float)r[c];
    }
  }
}

// what the calling thread's last multigrid solve did with its guess (piso_mg_last_guess): 0 none given, 1 accepted, 2 rejected
static thread_local int tl_mg_last_guess = 0;

// the start of a solve: mg_init's launch without a guess, the three launches above with one (rc: what the cycle reads, fl32(r) beside r
// under the float32 cycle)
// (the partial maxima use slots no kernel has pending then: part_max, which iteration 1 overwrites, and the fourth quarter of `parts`)
template <typename C>
static void mg_start(const Lv& L0, const double* divergence, const double* x0, double* x, double* r, C* rc, const double* scal, double* parts,
                     double* part_max, float accuracy, MgState* st, hipStream_t stream) {
  const int g0 = grid_for(L0.n, kBlock, kMgGrid);
  if (!x0) { mg_init<C><<<g0, kBlock, 0, stream>>>(L0, divergence, x, r, scal, rc); return; }
  double* part_b = parts + 3 * kMgGrid;
  mg_guess_residual<<<g0, kBlock, 0, stream>>>(L0, divergence, x0, r, scal, part_max, part_b, st);
  mg_guess_pick<<<1, kBlock, 0, stream>>>(part_max, part_b, g0, accuracy, st);
  mg_guess_apply<C><<<g0, kBlock, 0, stream>>>(L0, divergence, x0, x, r, scal, st, rc);
}
// ... and what the host's last look says the device did with the guess
static void mg_guess_record(const double* x0, const MgState* pinned) {
  tl_mg_last_guess = !x0 ? 0 : (pinned->flags & MG_FLAG_GUESS_REJECTED) ? 2 : 1;
}

}  // namespace piso
