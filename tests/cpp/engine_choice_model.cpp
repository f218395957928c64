// tests/test_engine_choice.py: the engine choice of UpdateESDF on the CPU.  This file includes the very header that
// dense_map.hip, hash_map.hip and shard_group.hip include and exposes its functions to ctypes, row by row.
//   g++ -std=c++17 -O2 -ffp-contract=off -fPIC -shared -o libengine_choice_model.so engine_choice_model.cpp
#include "../../fiesta_amd/csrc/engine_choice.hpp"

using namespace fiesta;

extern "C" {

int engine_choice_bulk_pays(double delta, double nocc, double n, double ft_last_ms, double bulk_ratio) {
  return bulk_pays_model(delta, nocc, n, ft_last_ms, bulk_ratio) ? 1 : 0;
}

// rows: 15 doubles each, in UpdateFacts' order (every value is an integer a double holds exactly, or a double);
// out: 4 words per row -- try_levels, try_bulk, ask_masked, notes
void engine_choice_rows(const double *rows, int64_t nrows, int32_t *out) {
  for (int64_t i = 0; i < nrows; ++i) {
    const double *r = rows + 15 * i;
    UpdateFacts f{};
    f.ni = (unsigned long long)r[0], f.nd = (unsigned long long)r[1];
    f.nocc = (long long)r[2], f.observed = (long long)r[3], f.owned = (long long)r[4], f.n = (long long)r[5];
    f.engine = (int)r[6];
    f.seed_only = r[7] != 0, f.sharded = r[8] != 0, f.wrap = r[9] != 0, f.gate_open = r[10] != 0;
    f.small_update = (long long)r[11], f.insert_cap = (long long)r[12];
    f.ft_last_ms = r[13], f.bulk_ratio = r[14];
    const EnginePlan p = choose_engines(f);
    out[4 * i] = p.try_levels, out[4 * i + 1] = p.try_bulk, out[4 * i + 2] = p.ask_masked, out[4 * i + 3] = (int32_t)p.notes;
  }
}

// 0: wanted, 1: engine or size rules it out, 2: density, 3: back-off by skip count, 4: back-off by last timings
int engine_choice_cells(int engine, int fits, long long nocc, long long n, int nn_skip, double nn_last_ms, double ft_last_ms, long long nn_last_nocc) {
  return (int)cells_verdict(engine, fits != 0, nocc, n, nn_skip, nn_last_ms, ft_last_ms, nn_last_nocc);
}

}  // extern "C"
