// Host driver of tests/test_mg_prepared_cpu.py: the two carves of a prepared multigrid solve and the one carve of the ordinary solve's
// workspace (csrc/mg_prepared_carve.h) are pure C++, so all can be walked without a card - against arenas WITHOUT memory (nothing is
// dereferenced).  Built with -fsanitize=address,undefined.
// Reads one query per line from stdin
//     nx ny elem            (elem 4: the float32 cycle, 8: the fp64 cycle)
// and prints: status (0 ok, 1 not a grid / precision the solver takes, 2 a check failed), the bytes of the hierarchy, the bytes of the scratch,
// the first failed check (- if none), and the bytes of the ordinary workspace.  Checks, for each carve: every array starts on a 256-byte boundary; the arrays do not overlap and end
// at the counted size; the counted size is mg_hier_bytes / mg_scratch_bytes; an arena of exactly that size is accepted and one byte less is
// refused; the levels have the dimensions of mg_dims; every float row of a level with nx % 4 == 0 is 16-byte aligned.  Across the two: laid out
// one after the other in one address space, no array of the scratch touches the hierarchy; the fp64 cycle's level 0 and outer r are lv[0] and
// r[0], the float32 cycle's are arrays of their own.  The ordinary workspace: the same checks of its one carve against mg_plan_bytes, no header,
// the hierarchy's sums in the solve's `scal`, the same aliasing of level 0 and the outer r.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "../differentiable-piso_amd/csrc/mg_prepared_carve.h"

namespace {

struct CheckedArena {                    // the interface of Arena (piso_common.h) and a record of every take
  char* base;
  size_t size, used;
  std::vector<std::pair<size_t, size_t>> takes;      // offset, bytes
  CheckedArena(uintptr_t p, size_t n) : base(reinterpret_cast<char*>(p)), size(n), used(0) {}
  template <typename T>
  T* take(size_t count) {
    used = (used + 255) / 256 * 256;
    takes.push_back({used, count * sizeof(T)});
    T* p = reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(base) + used);
    used += count * sizeof(T);
    return p;
  }
  bool ok() const { return used <= size; }
};

bool tidy(const CheckedArena& ar, std::string* why) {
  auto sorted = ar.takes;
  std::sort(sorted.begin(), sorted.end());
  for (size_t i = 0; i < sorted.size(); ++i) {
    if (sorted[i].first % 256) { *why = "an array does not start on a 256-byte boundary"; return false; }
    if (i + 1 < sorted.size() && sorted[i].first + sorted[i].second > sorted[i + 1].first) { *why = "two arrays overlap"; return false; }
  }
  if (sorted.empty() || sorted.back().first + sorted.back().second != ar.used) { *why = "the last array does not end at the counted size"; return false; }
  return true;
}

template <typename C>
int walk(int nx, int ny, size_t* hier_bytes, size_t* scratch_bytes, std::string* why) {
  const int elem = (int)sizeof(C);
  const uintptr_t base = 256;
  CheckedArena ah(base, ~(size_t)0);
  piso::MgHierT<C> H;
  if (!piso::mg_hier_carve(nx, ny, 1, 0, ah, H)) { *why = "the counting walk of the hierarchy failed"; return 2; }
  const uintptr_t sbase = base + (ah.used + 255) / 256 * 256;          // the scratch right behind the hierarchy
  CheckedArena as(sbase, ~(size_t)0);
  piso::MgScratchT<C> S;
  if (!piso::mg_scratch_carve(nx, ny, as, S)) { *why = "the counting walk of the scratch failed"; return 2; }
  *hier_bytes = ah.used; *scratch_bytes = as.used;
  if (!tidy(ah, why) || !tidy(as, why)) return 2;
  if (ah.used != piso::mg_hier_bytes(nx, ny, elem)) { *why = "the hierarchy's walk and mg_hier_bytes disagree"; return 2; }
  if (as.used != piso::mg_scratch_bytes(nx, ny, elem)) { *why = "the scratch's walk and mg_scratch_bytes disagree"; return 2; }
  const piso::MgDims d = piso::mg_dims(nx, ny);
  if (H.nlev != d.nlev || H.tail_first != d.tail_first) { *why = "the hierarchy's levels are not mg_dims'"; return 2; }
  const uintptr_t hend = base + ah.used, send = sbase + as.used;
  auto inside = [](const void* p, size_t bytes, uintptr_t lo, uintptr_t hi) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    return a >= lo && a + bytes <= hi;
  };
  if (!inside(H.hdr, sizeof(piso::MgHierHeader), base, hend) || !inside(H.scal, piso::SC_COUNT_MG * 8, base, hend)) { *why = "the header or the sums lie outside the hierarchy"; return 2; }
  if (H.L0.nx != nx || H.L0.ny != ny || H.L0.n != nx * ny || H.L0.per_x != 1 || H.L0.per_y != 0) { *why = "the fp64 level 0 has other dimensions"; return 2; }
  for (int l = 0; l < d.nlev; ++l) {
    const auto& L = H.lv[l];
    if (L.nx != d.nx[l] || L.ny != d.ny[l] || L.n != L.nx * L.ny || L.per_x != 1 || L.per_y != 0) { *why = "a level's dimensions are not the plan's"; return 2; }
    const size_t bytes = (size_t)L.n * sizeof(C);
    const C* hier[6] = {L.c[0], L.c[1], L.c[2], L.c[3], L.c[4], L.dinv};
    const C* scr[3] = {S.r[l], S.z[l], S.t[l]};
    for (const C* a : hier)
      if (!inside(a, bytes, base, hend)) { *why = "a level array lies outside the hierarchy"; return 2; }
    for (const C* a : scr)
      if (!inside(a, bytes, sbase, send)) { *why = "a vector of the cycle lies outside the scratch"; return 2; }
    if (sizeof(C) == 4 && L.nx % 4 == 0)
      for (int j = 0; j < L.ny; ++j) {
        for (const C* a : hier)
          if ((reinterpret_cast<uintptr_t>(a) + (size_t)j * L.nx * sizeof(C)) % 16) { *why = "a float row of a quad level is not 16-byte aligned"; return 2; }
        for (const C* a : scr)
          if ((reinterpret_cast<uintptr_t>(a) + (size_t)j * L.nx * sizeof(C)) % 16) { *why = "a float row of a quad level is not 16-byte aligned"; return 2; }
      }
  }
  const size_t n0 = (size_t)nx * ny * 8;
  const double* outer[6] = {H.L0.c[0], H.L0.c[1], H.L0.c[2], H.L0.c[3], H.L0.c[4], H.L0.dinv};
  for (const double* a : outer)
    if (!inside(a, n0, base, hend)) { *why = "the fp64 level 0 lies outside the hierarchy"; return 2; }
  const double* vec[4] = {S.r64, S.p[0], S.p[1], S.q};
  for (const double* a : vec)
    if (!inside(a, n0, sbase, send)) { *why = "an outer vector lies outside the scratch"; return 2; }
  if (!inside(S.parts, 4 * piso::kMgGrid * 8, sbase, send) || !inside(S.part_rz, piso::kMgGrid * 8, sbase, send) || !inside(S.part_pq, piso::kMgGrid * 8, sbase, send) ||
      !inside(S.part_max, piso::kMgGrid * 8, sbase, send) || !inside(S.scal, piso::SC_COUNT_MG * 8, sbase, send) || !inside(S.st, sizeof(piso::MgState), sbase, send)) {
    *why = "the partials, the sums or the state lie outside the scratch"; return 2;
  }
  const bool aliased = reinterpret_cast<const void*>(H.L0.c[2]) == reinterpret_cast<const void*>(H.lv[0].c[2]);
  const bool r_aliased = reinterpret_cast<const void*>(S.r64) == reinterpret_cast<const void*>(S.r[0]);
  if (sizeof(C) == 8 && (!aliased || !r_aliased)) { *why = "the fp64 cycle's level 0 / outer r are not lv[0] / r[0]"; return 2; }
  if (sizeof(C) == 4 && (aliased || r_aliased)) { *why = "the float32 cycle's fp64 level 0 / outer r share storage with the float32 arrays"; return 2; }
  // exactly the counted sizes are enough, one byte less is not
  piso::MgHierT<C> H2;
  piso::MgScratchT<C> S2;
  CheckedArena he(base, ah.used), hs(base, ah.used - 1), se(sbase, as.used), ss(sbase, as.used - 1);
  if (!piso::mg_hier_carve(nx, ny, 0, 0, he, H2) || !piso::mg_scratch_carve(nx, ny, se, S2)) { *why = "an arena of the counted size is refused"; return 2; }
  if (piso::mg_hier_carve(nx, ny, 0, 0, hs, H2) || piso::mg_scratch_carve(nx, ny, ss, S2)) { *why = "an arena one byte short is accepted"; return 2; }
  return 0;
}

// the one workspace of the ordinary solve
template <typename C>
int walk_plan(int nx, int ny, size_t* bytes, std::string* why) {
  const uintptr_t base = 256;
  CheckedArena aw(base, ~(size_t)0);
  piso::MgPlanT<C> P;
  if (!piso::mg_plan_carve(nx, ny, 1, 0, aw, P)) { *why = "the counting walk of the workspace failed"; return 2; }
  *bytes = aw.used;
  if (!tidy(aw, why)) return 2;
  if (aw.used != piso::mg_plan_bytes(nx, ny, (int)sizeof(C))) { *why = "the workspace's walk and mg_plan_bytes disagree"; return 2; }
  const piso::MgDims d = piso::mg_dims(nx, ny);
  if (P.H.nlev != d.nlev || P.H.tail_first != d.tail_first) { *why = "the workspace's levels are not mg_dims'"; return 2; }
  if (P.H.L0.nx != nx || P.H.L0.ny != ny || P.H.L0.n != nx * ny || P.H.L0.per_x != 1 || P.H.L0.per_y != 0) { *why = "the workspace's fp64 level 0 has other dimensions"; return 2; }
  for (int l = 0; l < d.nlev; ++l) {
    const auto& L = P.H.lv[l];
    if (L.nx != d.nx[l] || L.ny != d.ny[l] || L.n != L.nx * L.ny || L.per_x != 1 || L.per_y != 0) { *why = "a level of the workspace has not the plan's dimensions"; return 2; }
    const C* arr[9] = {L.c[0], L.c[1], L.c[2], L.c[3], L.c[4], L.dinv, P.S.r[l], P.S.z[l], P.S.t[l]};
    if (sizeof(C) == 4 && L.nx % 4 == 0)
      for (int j = 0; j < L.ny; ++j)
        for (const C* a : arr)
          if ((reinterpret_cast<uintptr_t>(a) + (size_t)j * L.nx * sizeof(C)) % 16) { *why = "a float row of a quad level of the workspace is not 16-byte aligned"; return 2; }
  }
  if (P.H.hdr != nullptr || P.H.scal != P.S.scal) { *why = "the ordinary workspace has a header or a second copy of the sums"; return 2; }
  const bool aliased = reinterpret_cast<const void*>(P.H.L0.c[2]) == reinterpret_cast<const void*>(P.H.lv[0].c[2]);
  const bool r_aliased = reinterpret_cast<const void*>(P.S.r64) == reinterpret_cast<const void*>(P.S.r[0]);
  if (sizeof(C) == 8 && (!aliased || !r_aliased)) { *why = "the fp64 cycle's level 0 / outer r are not lv[0] / r[0] in the workspace"; return 2; }
  if (sizeof(C) == 4 && (aliased || r_aliased)) { *why = "the float32 cycle's fp64 level 0 / outer r share storage with the float32 arrays in the workspace"; return 2; }
  piso::MgPlanT<C> P2;
  CheckedArena we(base, aw.used), wshort(base, aw.used - 1);
  if (!piso::mg_plan_carve(nx, ny, 0, 0, we, P2)) { *why = "a workspace of the counted size is refused"; return 2; }
  if (piso::mg_plan_carve(nx, ny, 0, 0, wshort, P2)) { *why = "a workspace one byte short is accepted"; return 2; }
  return 0;
}

}  // namespace

int main() {
  int nx, ny, elem;
  while (scanf("%d %d %d", &nx, &ny, &elem) == 3) {
    size_t hb = 0, sb = 0, wb = 0;
    int status = 1;
    std::string why = "-";
    if (piso::mg_hier_bytes(nx, ny, elem) != 0 && piso::mg_scratch_bytes(nx, ny, elem) != 0)
      status = elem == 4 ? walk<float>(nx, ny, &hb, &sb, &why) : walk<double>(nx, ny, &hb, &sb, &why);
    if (status == 0) status = elem == 4 ? walk_plan<float>(nx, ny, &wb, &why) : walk_plan<double>(nx, ny, &wb, &why);
    else if ((piso::mg_hier_bytes(nx, ny, elem) != 0) != (piso::mg_scratch_bytes(nx, ny, elem) != 0)) { status = 2; why = "one size is zero and the other is not"; }
    if ((status == 1) != (piso::mg_plan_bytes(nx, ny, elem) == 0)) { status = 2; why = "mg_plan_bytes and the prepared sizes disagree about what the solver takes"; }
    printf("%d\t%zu\t%zu\t%s\t%zu\n", status, hb, sb, why.c_str(), wb);
  }
  return 0;
}
