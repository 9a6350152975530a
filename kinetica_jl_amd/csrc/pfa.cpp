// Host tables of path flux analysis: the second-generation pattern E2 of a DRG pattern E, its sizes and the order of its
// rows by cost (pfa.hpp).
#include "pfa.hpp"

#include <algorithm>
#include <numeric>

namespace kin {

PfaTables build_pfa_tables(int64_t N, const std::vector<int32_t>& rowptr, const std::vector<int32_t>& colidx) {
  PfaTables t;
  t.N = N; t.E = (int64_t)colidx.size();
  t.rowptr2.assign((size_t)N + 1, 0);
  std::vector<int64_t> cost((size_t)N, 0);
  std::vector<int32_t> mark((size_t)N, -1), row;
  auto deg = [&](int64_t i) { return (int64_t)(rowptr[i + 1] - rowptr[i]); };
  for (int64_t A = 0; A < N; A++) {
    t.max_row = std::max(t.max_row, deg(A));
    row.clear();
    mark[A] = (int32_t)A;      // (no diagonal)
    auto add = [&](int32_t B) {
      if (mark[B] != (int32_t)A) { mark[B] = (int32_t)A; row.push_back(B); }
    };
    for (int32_t e = rowptr[A]; e < rowptr[A + 1]; e++) {
      const int32_t M = colidx[e];
      add(M);
      cost[A] += deg(M);
      for (int32_t f = rowptr[M]; f < rowptr[M + 1]; f++) add(colidx[f]);
    }
    t.products += cost[A];
    std::sort(row.begin(), row.end());
    if (t.colidx2.size() + row.size() >= ((size_t)1 << 31)) throw KinError(ERR_UNSUPPORTED, "PFA: second-generation pattern beyond 32-bit offsets");
    t.colidx2.insert(t.colidx2.end(), row.begin(), row.end());
    t.rowptr2[A + 1] = (int32_t)t.colidx2.size();
  }
  t.E2 = (int64_t)t.colidx2.size();
  for (int64_t A = 0; A < N; A++)
    if (deg(A) > 0) t.order.push_back((int32_t)A);
  std::stable_sort(t.order.begin(), t.order.end(), [&](int32_t x, int32_t y) { return cost[x] > cost[y]; });
  t.order_cost.reserve(t.order.size());
  for (int32_t A : t.order) t.order_cost.push_back(cost[A]);
  return t;
}

}  // namespace kin
