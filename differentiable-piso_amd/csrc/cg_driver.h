// The pressure CG's iteration, written once for the one-GPU solve (cg.hip: GpuLink) and the slab solve (cg_slab.hip: SlabLink):
//   cg_next_step      the schedule - pure, no HIP calls: which iterations run as one persistent segment, which one resets, the first;
//   cg_iterate        the one loop: owns the state version, the pending x update, the order of the steps.  Everything the two solves
//                     really differ in - launches, collectives, halo rows, the host's looks, verification - is its Link's;
//   cg_coefs          the one reading of the coefficient flags;  cg_with_instance: the one <CT, V, RECON> ladder;
//   cg_retry_without_segments   the second attempt on the two-kernel iteration after a persistent segment failed.
#pragma once
#include "cg_dispatch.h"

namespace piso {

// ---- the schedule.  From iteration k: NORMAL iterations [k, ke) in one persistent launch - up to the next reset iteration / the end
// / one segment length - or iteration k alone: a residual reset (every `reset`-th), the first, or a NORMAL one on the two-kernel path.
// fixed: the fixed-work mode of piso_cg_fixed_iterations (one GPU only) - no resets.
enum CgStepKind { CG_SEGMENT, CG_RESET, CG_FIRST, CG_NORMAL };
struct CgStep { CgStepKind kind; int ke; };
inline CgStep cg_next_step(int k, int total, int reset, bool fixed, int seg_len, bool persistent) {
  const bool is_reset = !fixed && ((k + 1) % reset == 0);
  if (persistent && k > 0 && !is_reset) {
    int ke = total;
    if (!fixed) { const int next_reset = ((k + 1 + reset - 1) / reset) * reset - 1; if (next_reset < ke) ke = next_reset; }
    if (ke > k + seg_len) ke = k + seg_len;
    if (ke > k) return {CG_SEGMENT, ke};
  }
  return {is_reset ? CG_RESET : (k == 0 ? CG_FIRST : CG_NORMAL), k + 1};
}

// ---- what cg_setup_coeffs found (cells whose off-diagonals are not exact floats / whose diagonal cannot be rebuilt from them / whose
// matrix is not symmetric; a slab passes the sums over all ranks) and the knobs cg_no_compact / cg_no_recon / cg_no_sym.
// The off-diagonals of the PISO pressure matrix are float32 face coefficients (laplace_op.cu.cc:140-177): stored as float they are
// exact and K1 reads 24 instead of 40 coefficient bytes per cell.  Any other input keeps them in T.
struct CgCoefs { bool compact, recon, symmetric; };
inline CgCoefs cg_coefs(double not_f32, double not_recon, double not_sym, bool no_compact, bool no_recon, bool no_sym) {
  CgCoefs c;
  c.compact = not_f32 == 0 && !no_compact;
  c.recon = c.compact && not_recon == 0 && !no_recon;
  c.symmetric = not_sym == 0 && !no_sym;
  return c;
}

// ---- the ladder: calls f(CgInstance<CT, V, RECON>) for state type T (lanes of 16 bytes where `vec`) and returns what it returns
template <typename CT_, int V_, bool RECON_>
struct CgInstance { using CT = CT_; static constexpr int V = V_; static constexpr bool RECON = RECON_; };
template <typename T, typename F>
inline int cg_with_instance(const CgCoefs& c, bool vec, F&& f) {
  constexpr int VMID = 16 / sizeof(T);
  if (c.compact && c.recon) return vec ? f(CgInstance<float, VMID, true>{}) : f(CgInstance<float, 1, true>{});
  if (c.compact) return vec ? f(CgInstance<float, VMID, false>{}) : f(CgInstance<float, 1, false>{});
  return vec ? f(CgInstance<T, VMID, false>{}) : f(CgInstance<T, 1, false>{});
}

// ---- attempt(allow_persist) returns PISO_OK, an error, or kPersistRetry: a persistent segment failed (an exchange gave up: some
// workgroups were not resident - another kernel or process holds CUs; or the true-residual check) and its state is unusable.  Then
// the whole solve runs again on the two-kernel iteration, which needs no co-residency (the attempt re-initialises what it must).
template <typename F>
inline int cg_retry_without_segments(const char* who, F&& attempt) {
  for (int i = 0; i < 2; ++i) {
    const int rc = attempt(i == 0);
    if (rc != kPersistRetry) return rc;
  }
  char msg[96];
  snprintf(msg, sizeof(msg), "%s: persistent segment failed twice", who);
  set_error_msg(msg);
  return PISO_ERR_HIP;
}

// ---- workspace sizes are counted by running a solve's carve against an arena without memory.  The slack is what the hand-written
// formulas of old advertised beyond their carves (the set-up partials at three times their size, the four off-diagonal arrays rounded
// one by one, 4.5 KiB of margin), rounded up: callers cache workspaces by size, so no shape is advertised less than it ever was.
constexpr size_t kCgWsSlack = 40 * 1024;
inline Arena counting_arena() { return Arena(nullptr, ~(size_t)0); }
inline size_t counted_bytes(const Arena& ar) { return align_up(ar.used, 256) + kCgWsSlack; }

// ---- the loop.  A Link provides (int status each; k: iteration, sv: state version):
//   persistent(), seg_len      can NORMAL iterations run in persistent launches, and how many in one
//   segment(k, ke, st)         one launch of [k, ke) and what follows it; sets st.finished / st.stop_it; kPersistRetry if it failed
//   k1(k, mode, sv, chk, pend), k2(k, sv), flush(k, sv), reset_residual(sv)    the kernels of the two-kernel iteration
//   halo(which)                neighbours' edge rows of HALO_R / HALO_X (slabs)
//   look(k, st)                the host's stopping look after iteration k
//   finish(st)                 the last look, verification, copies; kPersistRetry if the solve must run again
enum { HALO_R = 0, HALO_X = 1 };
struct CgLoop {
  int total;                                             // iterations at most
  int sv = 0, k_last = -1, stop_it = -1, segments_run = 0;
  bool pending = false;                                  // x still lacks alpha_k p_k of the last executed iteration
  bool finished = false;
};

template <typename Link>
inline int cg_iterate(Link& link, int total, int reset, bool fixed, int* iterations_out) {
  CgLoop st;
  st.total = total;
  for (int k = 0; k < total && !st.finished;) {
    const CgStep step = cg_next_step(k, total, reset, fixed, link.seg_len, link.persistent());
    if (step.kind == CG_SEGMENT) {
      PISO_TRY(link.segment(k, step.ke, st));
      ++st.segments_run;
      st.k_last = step.ke - 1;
      st.pending = false;                                // the segment applies every x += alpha p itself
      k = step.ke;
      continue;
    }
    if (step.kind == CG_RESET) {
      if (st.pending) { PISO_TRY(link.flush(k - 1, st.sv)); st.pending = false; }
      PISO_TRY(link.halo(HALO_X));                       // for L x
      PISO_TRY(link.k1(k, MODE_RESET, st.sv, k > 0 ? 1 : 0, 0));
      ++st.sv;
      PISO_TRY(link.reset_residual(st.sv));
      PISO_TRY(link.halo(HALO_R));
      PISO_TRY(link.k1(k, MODE_INIT, st.sv, 0, 0));
    } else if (step.kind == CG_FIRST) {
      PISO_TRY(link.k1(k, MODE_INIT, st.sv, 0, 0));
    } else {
      PISO_TRY(link.k1(k, MODE_NORMAL, st.sv, 1, st.pending ? 1 : 0));
      ++st.sv;
    }
    PISO_TRY(link.k2(k, st.sv));
    PISO_TRY(link.halo(HALO_R));                         // of the new residual
    PISO_LAUNCH_CHECK();
    st.pending = true;
    st.k_last = k;
    PISO_TRY(link.look(k, st));
    ++k;
  }
  // the direction of the last executed iteration (a converged solve was already flushed by the K1 that detected it)
  if (st.pending && st.k_last >= 0) PISO_TRY(link.flush(st.k_last, st.sv));
  PISO_TRY(link.finish(st));
  if (iterations_out) *iterations_out = st.finished ? st.stop_it : total;
  return PISO_OK;
}

}  // namespace piso
