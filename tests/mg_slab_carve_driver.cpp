// Host driver of tests/test_mg_slab_f32_cpu.py: the workspace carve of the slab multigrid (csrc/mg_slab_carve.h) is pure C++, so a rank's share
// can be walked without a card - against an arena WITHOUT memory (base 256, nothing is dereferenced).  Built with -fsanitize=address,undefined.
// Reads one query per line from stdin
//     nx ny world gather_cells elem            (elem 4: the float32 cycle, 8: the fp64 cycle)
// and prints: status (0 ok, 1 plan refused, 2 a check failed), bytes of the rank's share, the number of float row pointers checked, and the
// first failed check (- if none).  Checks: every array starts on a 256-byte boundary of the arena (before the halo offset); every float row
// pointer of a level whose nx is a multiple of four - halo offset included, and the halo rows -1 and ny themselves - is 16-byte aligned; the
// arrays do not overlap and lie inside the counted size; the walk against an arena of exactly that size succeeds and one byte less fails.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "../differentiable-piso_amd/csrc/mg_slab_carve.h"

namespace {

struct CheckedArena {                    // the interface of Arena (piso_common.h) and a record of every take
  char* base;
  size_t size, used;
  std::vector<std::pair<size_t, size_t>> takes;      // offset, bytes
  CheckedArena(void* p, size_t n) : base(static_cast<char*>(p)), size(n), used(0) {}
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

template <typename C>
int walk(const piso::MgSlabPlan& sp, size_t* bytes, int* rows_checked, std::string* why) {
  CheckedArena ar(reinterpret_cast<void*>(256), ~(size_t)0);
  piso::MgSlabRankT<C> k;
  if (!piso::mg_slab_carve(sp, 1, 1, ar, k)) { *why = "the counting walk failed"; return 2; }
  *bytes = ar.used;
  auto sorted = ar.takes;
  std::sort(sorted.begin(), sorted.end());
  for (size_t i = 0; i < sorted.size(); ++i) {
    if (sorted[i].first % 256) { *why = "an array does not start on a 256-byte boundary"; return 2; }
    if (i + 1 < sorted.size() && sorted[i].first + sorted[i].second > sorted[i + 1].first) { *why = "two arrays overlap"; return 2; }
  }
  if (sorted.back().first + sorted.back().second != ar.used) { *why = "the last array does not end at the counted size"; return 2; }
  *rows_checked = 0;
  for (int l = 0; l < sp.d.nlev; ++l) {
    const auto& L = k.lv[l];
    const bool sharded = l < sp.g;
    if (L.nx != sp.d.nx[l] || L.ny != sp.rows[l] || L.n != L.nx * L.ny) { *why = "a level's dimensions are not the plan's"; return 2; }
    const C* arrays[9] = {L.c[0], L.c[1], L.c[2], L.c[3], L.c[4], L.dinv, k.r[l], k.z[l], k.t[l]};
    for (const C* a : arrays) {
      const uintptr_t first = reinterpret_cast<uintptr_t>(a) - (sharded ? (uintptr_t)L.nx * sizeof(C) : 0);      // the halo row below, or row 0
      if (first % 256) { *why = "a level array does not start on the arena's boundary"; return 2; }
      if (sizeof(C) == 4 && L.nx % 4 == 0)
        for (int j = sharded ? -1 : 0; j < L.ny + (sharded ? 1 : 0); ++j) {
          if ((reinterpret_cast<uintptr_t>(a) + (intptr_t)j * L.nx * (intptr_t)sizeof(C)) % 16) { *why = "a float row of a quad level is not 16-byte aligned"; return 2; }
          ++*rows_checked;
        }
    }
  }
  if (sizeof(C) == 4) {
    if (!k.L0.c[0] || !k.L0.dinv || k.L0.n != sp.d.nx[0] * sp.nyl) { *why = "the float32 cycle has no fp64 level 0"; return 2; }
    if (reinterpret_cast<void*>(k.ro) == reinterpret_cast<void*>(k.r[0])) { *why = "the outer r shares storage with fl32(r)"; return 2; }
  } else if (sp.g > 0 && reinterpret_cast<void*>(k.ro) != reinterpret_cast<void*>(k.r[0])) {
    *why = "the fp64 cycle's outer r is not r[0]"; return 2;
  }
  const uintptr_t rows0[3] = {reinterpret_cast<uintptr_t>(k.p[0]), reinterpret_cast<uintptr_t>(k.p[1]), reinterpret_cast<uintptr_t>(k.x)};
  for (uintptr_t p : rows0)
    if ((p - (uintptr_t)sp.d.nx[0] * 8) % 256) { *why = "p / x do not start on the arena's boundary"; return 2; }
  // exactly the counted size is enough, one byte less is not
  CheckedArena exact(reinterpret_cast<void*>(256), ar.used), small(reinterpret_cast<void*>(256), ar.used - 1);
  piso::MgSlabRankT<C> k2;
  if (!piso::mg_slab_carve(sp, 0, 0, exact, k2)) { *why = "an arena of the counted size is refused"; return 2; }
  if (piso::mg_slab_carve(sp, 0, 0, small, k2)) { *why = "an arena one byte short is accepted"; return 2; }
  return 0;
}

}  // namespace

int main() {
  int nx, ny, world, knob, elem;
  while (scanf("%d %d %d %d %d", &nx, &ny, &world, &knob, &elem) == 5) {
    const piso::MgSlabPlan sp = piso::mg_slab_plan(nx, ny, world, knob);
    size_t bytes = 0;
    int rows = 0, status = 1;
    std::string why = "-";
    if (sp.status == 0) status = elem == 4 ? walk<float>(sp, &bytes, &rows, &why) : walk<double>(sp, &bytes, &rows, &why);
    printf("%d\t%zu\t%d\t%s\n", status, bytes, rows, why.c_str());
  }
  return 0;
}
