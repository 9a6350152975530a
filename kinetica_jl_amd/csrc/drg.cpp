// Host tables of the directed-relation-graph pass: edge CSR, contribution lists, gather plans (drg.hpp).
#include "drg.hpp"

#include <algorithm>

namespace kin {

namespace {

struct Contrib { int32_t A, B, kf, kr; float c, s; };   // c = |nu_A|, s = nu_A

// the plan's coefficients by payload slot (ELL slots first, the medium and long rows' payload behind them)
void place_coefs(const SegPlanHost& p, const std::vector<int32_t>& slot, const std::vector<float>& c, std::vector<float>& ell_c,
                 std::vector<float>& long_c) {
  ell_c.assign((size_t)p.ell_total, 0.0f);
  long_c.assign((size_t)p.long_total, 0.0f);
  for (size_t e = 0; e < slot.size(); e++) {
    if (slot[e] < 0) continue;
    if (slot[e] < p.ell_total) ell_c[slot[e]] = c[e]; else long_c[slot[e] - p.ell_total] = c[e];
  }
}

void classify(const std::vector<int32_t>& ptr, int64_t cls[3]) {
  for (size_t i = 0; i + 1 < ptr.size(); i++) {
    const int32_t len = ptr[i + 1] - ptr[i];
    cls[len <= SegPlanHost::SHORT_MAX ? 0 : (len <= SegPlanHost::SEG_LEN ? 1 : 2)]++;
  }
}

}  // namespace

DrgTables build_drg_tables(const NetworkHost& h, int pairing, bool with_plans, bool with_edges) {
  DrgTables t;
  const int64_t N = h.N, R = h.R;
  t.N = N;
  if (pairing && R > 0 && h.pair_k.empty()) throw KinError(ERR_UNSUPPORTED, "DRG with pairing needs the pair records (N < 65535)");
  const int64_t n_rec = pairing ? h.n_pairs() : R;
  std::vector<Contrib> den, num;
  den.reserve((size_t)n_rec * 4);
  if (with_edges) num.reserve((size_t)n_rec * 12);
  for (int64_t p = 0; p < n_rec; p++) {
    const int32_t kf = pairing ? h.pair_k[2 * p] : (int32_t)p, kr = pairing ? h.pair_k[2 * p + 1] : -1;
    int32_t S[6]; int nS = 0;
    auto add = [&](int32_t sp) {
      if (sp < 0) return;
      for (int j = 0; j < nS; j++) if (S[j] == sp) return;
      S[nS++] = sp;
    };
    add(h.x0[kf]); add(h.x1[kf]);
    for (int j = 0; j < 4; j++) add(h.slot_sp[4 * kf + j]);
    for (int j = 0; j < 4; j++) {
      const int32_t A = h.slot_sp[4 * kf + j];
      if (A < 0) continue;
      const int nu = (int)(int8_t)((uint32_t)h.slot_co[kf] >> (8 * j));
      const float c = (float)(nu < 0 ? -nu : nu);
      den.push_back({A, -1, kf, kr, c, (float)nu});
      for (int q = 0; q < nS && with_edges; q++) if (S[q] != A) num.push_back({A, S[q], kf, kr, c, (float)nu});
    }
  }
  // (stable: the contributions of a row / an edge stay in record order)
  std::stable_sort(den.begin(), den.end(), [](const Contrib& x, const Contrib& y) { return x.A < y.A; });
  std::stable_sort(num.begin(), num.end(), [](const Contrib& x, const Contrib& y) { return x.A != y.A ? x.A < y.A : x.B < y.B; });
  if (num.size() >= ((size_t)1 << 31)) throw KinError(ERR_UNSUPPORTED, "DRG: contribution lists beyond 32-bit offsets");
  t.n_den = (int64_t)den.size(); t.n_num = (int64_t)num.size();
  std::vector<int32_t> den_ptr((size_t)N + 1, 0), edge_ptr(1, 0), edge_row;
  for (const Contrib& d : den) den_ptr[d.A + 1]++;
  for (int64_t i = 0; i < N; i++) den_ptr[i + 1] += den_ptr[i];
  t.rowptr.assign((size_t)N + 1, 0);
  for (size_t e = 0; e < num.size(); e++) {
    if (e == 0 || num[e].A != num[e - 1].A || num[e].B != num[e - 1].B) {
      if (e > 0) edge_ptr.push_back((int32_t)e);
      t.colidx.push_back(num[e].B);
      edge_row.push_back(num[e].A);
      t.rowptr[num[e].A + 1]++;
    }
  }
  if (!num.empty()) edge_ptr.push_back((int32_t)num.size());
  for (int64_t i = 0; i < N; i++) t.rowptr[i + 1] += t.rowptr[i];
  t.E = (int64_t)t.colidx.size();
  classify(den_ptr, t.den_cls);
  classify(edge_ptr, t.edge_cls);
  if (!with_plans) return t;
  auto plan = [&](const std::vector<Contrib>& v, const std::vector<int32_t>& ptr, const int32_t* aux, SegPlanHost& out,
                  std::vector<float>& ell_c, std::vector<float>& long_c, std::vector<float>& ell_s, std::vector<float>& long_s) {
    std::vector<int32_t> a(v.size()), b(v.size()), slot;
    std::vector<float> c(v.size()), sg(v.size());
    for (size_t e = 0; e < v.size(); e++) { a[e] = v[e].kf; b[e] = v[e].kr; c[e] = v[e].c; sg[e] = v[e].s; }
    out = build_seg_plan((int64_t)ptr.size() - 1, ptr.data(), nullptr, a.data(), b.data(), nullptr, false, aux, &slot);
    place_coefs(out, slot, c, ell_c, long_c);
    place_coefs(out, slot, sg, ell_s, long_s);
  };
  plan(den, den_ptr, nullptr, t.den_plan, t.den_ell_c, t.den_long_c, t.den_ell_s, t.den_long_s);
  if (!with_edges) { t.have_plans = true; return t; }
  plan(num, edge_ptr, edge_row.data(), t.edge_plan, t.edge_ell_c, t.edge_long_c, t.edge_ell_s, t.edge_long_s);
  // the transpose of the pattern (a counting sort by head: the sources of a species stay ascending)
  t.in_ptr.assign((size_t)N + 1, 0);
  for (int64_t e = 0; e < t.E; e++) t.in_ptr[t.colidx[e] + 1]++;
  for (int64_t i = 0; i < N; i++) t.in_ptr[i + 1] += t.in_ptr[i];
  t.in_src.resize((size_t)t.E); t.in_edge.resize((size_t)t.E);
  {
    std::vector<int32_t> fill(t.in_ptr.begin(), t.in_ptr.end() - 1);
    for (int64_t A = 0; A < N; A++)
      for (int32_t e = t.rowptr[A]; e < t.rowptr[A + 1]; e++) {
        const int32_t j = fill[t.colidx[e]]++;
        t.in_src[j] = (int32_t)A; t.in_edge[j] = e;
      }
  }
  auto in_class = [&](int64_t i) {
    const int32_t len = t.in_ptr[i + 1] - t.in_ptr[i];
    return len <= DrgTables::IN_SHORT_MAX ? 0 : (len <= DrgTables::IN_WAVE_MAX ? 1 : 2);
  };
  t.in_order.reserve((size_t)N);
  for (int c = 0; c < 3; c++)
    for (int64_t i = 0; i < N; i++)
      if (in_class(i) == c) { t.in_order.push_back((int32_t)i); t.in_cls[c]++; }
  t.have_plans = true;
  return t;
}

RiTables build_ri_tables(const NetworkHost& h, int pairing) {
  RiTables t;
  const int64_t R = h.R;
  t.R = R;
  if (pairing && R > 0 && h.pair_k.empty()) throw KinError(ERR_UNSUPPORTED, "reaction importance with pairing needs the pair records (N < 65535)");
  t.n_records = pairing ? h.n_pairs() : R;
  t.partner.assign((size_t)R, -1);
  t.species.assign((size_t)4 * R, -1);
  t.nu.assign((size_t)4 * R, 0);
  for (int64_t p = 0; p < t.n_records; p++) {
    const int32_t kf = pairing ? h.pair_k[2 * p] : (int32_t)p, kr = pairing ? h.pair_k[2 * p + 1] : -1;
    if (kr >= 0) { t.partner[kf] = kr; t.partner[kr] = kf; t.n_paired += 2; }
    bool any = false;
    for (int j = 0; j < 4; j++) {
      const int32_t A = h.slot_sp[4 * kf + j];
      if (A < 0) continue;
      const int nu = (int)(int8_t)((uint32_t)h.slot_co[kf] >> (8 * j));
      t.species[4 * kf + j] = A; t.nu[4 * kf + j] = nu;
      if (kr >= 0) { t.species[4 * kr + j] = A; t.nu[4 * kr + j] = -nu; }
      any = any || nu != 0;
    }
    if (!any) t.n_empty += kr >= 0 ? 2 : 1;
  }
  return t;
}

std::vector<int32_t> RiTables::dev() const {
  std::vector<int32_t> d((size_t)6 * R, 0);
  for (int64_t r = 0; r < R; r++) {
    d[r] = partner[r];
    uint32_t co = 0;
    for (int j = 0; j < 4; j++) {
      const int32_t c = nu[4 * r + j];
      d[(size_t)(1 + j) * R + r] = c != 0 ? species[4 * r + j] : -1;
      co |= (uint32_t)(c < 0 ? -c : c) << (8 * j);
    }
    d[(size_t)5 * R + r] = (int32_t)co;
  }
  return d;
}

}  // namespace kin
