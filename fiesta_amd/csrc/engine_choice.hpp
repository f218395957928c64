// Which engines an UpdateESDF tries, as pure functions of a few numbers: the definition of the choice for the dense store
// (dense_map.hip: update_esdf), the hash store (hash_map.hip) and the sharded driver (shard_group.hip).  Host-only, no HIP:
// tests/cpp/engine_choice_model.cpp compiles this very header with g++ and tests/test_engine_choice.py sweeps it.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>

#include "../../include/fiesta_hip.h"

namespace fiesta {
// The cost half of the engine choice, from the measured crossover (profiles/r03a_delta_sweep.json: C2's map, both scenes,
// deltas 100 ... 50 k on either engine).  The transform is one fixed sweep, ~6 ps per voxel of the grid; the rounds cost a
// fixed ~0.8 ms of launches and scans on a 512^3 map plus ~0.3 ns per voxel whose obstacle changes, about
// delta x (voxels per obstacle) of them.  In voxel units: bulk pays iff  n <= 1.3e8 + 50 x (estimated updated voxels) --
// on every grid up to 512^3 that is always (measured: 0.80 vs 0.93 ms at a delta of 100), on a 1024^3 shard from a delta of
// ~2 % of the obstacles.  FIESTA_HIP_BULK_RATIO (a fraction of the occupied voxels) overrides the model.
// (a free function of its arguments: the sharded driver decides from numbers every rank has seen -- the gathered maxima --
//  never from one rank's own)
inline bool bulk_pays_model(double delta, double nocc, double n, double ft_last_ms, double bulk_ratio) {
  if (bulk_ratio >= 0) return delta >= bulk_ratio * std::max(nocc, 1.0);
  const double updated = std::min(n, delta * n / std::max(nocc, 1.0));
  // a scene of deep deques (surfaces: the transform takes twice the sweep's nominal time) and a handful of voxels: the
  // rounds win by a few percent (measured: 1.38 vs 1.53 ms at a delta of 100, 2.1 vs 1.5 ms at 500)
  if (delta <= 128 && ft_last_ms > 1.25 * n * 6e-9) return false;
  return n <= 1.3e8 + 50.0 * updated;
}

struct UpdateFacts {  // what the choice reads, and nothing else
  unsigned long long ni, nd;           // lengths of the insert and delete queues
  long long nocc, observed, owned, n;  // occupied / observed voxels, voxels this map owns, voxels of the array
  int engine;                          // update_engine, 0 ... 6
  bool seed_only, sharded, wrap;
  bool gate_open;  // the map's state allows an exact transform (DenseMap::bulk_eligible, asked only if !seed_only && !sharded)
  long long small_update, insert_cap;  // the level engine's share: inserts + deletes, inserts
  double ft_last_ms, bulk_ratio;       // bulk_pays_model's
};
// ask_masked: the masked transform, if DenseMap::masked_eligible agrees (it may launch: asked only when this is set);
// notes: FIESTA_HIP_NOTE_*, the standing conditions and SMALL_DELTA
struct EnginePlan { bool try_levels, try_bulk, ask_masked; uint32_t notes; };

// The bulk transform costs one fixed sweep over the grid; the frontier rounds cost in proportion to the voxels whose closest
// obstacle changes, roughly (inserts + deletes) x (grid / occupied voxels).  The level engine (level_kernels.hpp) takes every
// update of a few thousand voxels -- a sensor frame -- that the transform does not, and, if asked for (update_engine 3), every
// update its lists can hold; one that outgrows them is finished by the rounds.
inline EnginePlan choose_engines(const UpdateFacts &f) {
  const bool pinned = f.engine == 2 || f.engine == 4 || f.engine == 5;  // (DenseMap::bulk_pinned)
  const bool pays = bulk_pays_model((double)(f.ni + f.nd), (double)f.nocc, (double)f.n, f.ft_last_ms, f.bulk_ratio);
  EnginePlan p{};
  // On a map the transform's gate is open for -- every voxel observed, no history of partial windows -- the reference's
  // field is the exact transform whatever the order (section 3c): the level engine has nothing to add there, and a delete on
  // such a map orphans a whole Voronoi cell (10^5 voxels behind a surface), which is the rounds' or the transform's work.
  // (the inserts ARE level 0: more of them than one work-group carries and the level engine would only hand the update on)
  p.try_levels = !f.seed_only && !f.sharded && !f.wrap && f.engine != 1 &&
                 (f.engine == 3 || (!f.gate_open && f.ni + f.nd <= (unsigned long long)f.small_update && f.ni <= (unsigned long long)f.insert_cap));
  p.try_bulk = f.gate_open && (pinned || pays);
  // A partially observed map (every map a sensor builds): a delta too large for the level engine goes to the masked transform
  // (mask_kernels.hpp) where the map's history allows it -- a fixed sweep like the other transforms -- instead of the rounds.
  p.ask_masked = !f.seed_only && !f.gate_open && f.observed < f.n &&
                 (f.engine == 6 || (!p.try_levels && (f.engine == 0 || pinned) && pays));
  // why this update will take the path it takes (fiesta_hip_stats.path_notes): the standing conditions here, the rest as they bite
  if (f.observed != f.owned) p.notes |= FIESTA_HIP_NOTE_PARTLY_OBSERVED;
  if (f.sharded) p.notes |= FIESTA_HIP_NOTE_SHARDED;
  if (f.wrap) p.notes |= FIESTA_HIP_NOTE_ID_WRAP;
  if (f.engine != 0) p.notes |= FIESTA_HIP_NOTE_ENGINE_PINNED;
  if (f.gate_open ? !p.try_bulk : !f.seed_only && f.observed < f.n && !pinned && !pays) p.notes |= FIESTA_HIP_NOTE_SMALL_DELTA;
  return p;
}

// Whether the cell transform (nn_kernels.hpp) is worth trying before the envelope passes: the obstacle density must be in the
// range where every cell finds an obstacle within its search window and lists stay short (measured on scatter scenes,
// profiles/r05h_density_range.json: 8e-5 ... 2.5e-3 of the voxels; config 2's scene is 3.7e-4), it must not have failed at about
// this obstacle count, and it must not have been slower than the envelope passes.
enum class CellsVerdict { kWanted, kRuledOut /* engine or size */, kDensity, kSkipCount /* back-off */, kLastTimings /* back-off */ };
inline CellsVerdict cells_verdict(int engine, bool fits /* within nn::kRegionMax voxels per axis */, long long nocc, long long n, int nn_skip,
                                  double nn_last_ms, double ft_last_ms, long long nn_last_nocc) {
  if (engine == 4 || !fits) return CellsVerdict::kRuledOut;
  if (engine == 5) return CellsVerdict::kWanted;
  // (measured with the cells that get no list served one by one, profiles/r06_density_range.json: 7.5e-5 -- 0.36 against 0.57 ms on
  //  the envelope passes; 5.2e-5 -- two cells scan every site, 0.89 against 0.56; 2.5e-3 -- 0.74 against 0.98; 3.7e-3 -- 1.14 against 1.04)
  if (nocc * 15000 < n || nocc * 400 > n) return CellsVerdict::kDensity;
  // a failed attempt (a cell without a list: ~0.2 ms lost before the envelope passes take over) is not repeated at once: the
  // next 8, 16, ... 256 eligible updates go straight to the envelope passes, then it is tried again -- a scene that cannot be
  // served costs 1 % in the long run, one unlucky cell in a scene that can does not switch the transform off for good
  if (nn_skip > 0) return CellsVerdict::kSkipCount;
  if (nn_last_ms > 0 && ft_last_ms > 0 && nn_last_ms > ft_last_ms && std::llabs(nocc - nn_last_nocc) * 4 <= nn_last_nocc) return CellsVerdict::kLastTimings;
  return CellsVerdict::kWanted;
}

}  // namespace fiesta
