// prelude.hpp -- what every translation unit of the library starts with, in dependency order
//
// The library is built from several translation units compiled side by side (mmsbm_amd/build.py) and linked into one
// shared object:
//   mmsbm_hip.hip  the C ABI: argument checks and one call into the unit that owns the work
//   tu_create.hip  building a context: the shape plan, the index and its uploads, the per-restart state
//   tu_params.hip  parameters in and out: the host's arrays <-> the device's padded, split tables; snapshots
//   tu_iterate.hip the EM iteration: its form, its order of launches, graph replay, the timers; the launch log
//   tu_options.hip the option table
//   tu_seg.hip     the two triple passes (seg_pass.hpp)
//   tu_pair.hip    the pair stage on the vector ALUs (pair_block.hpp, pair_quad.hpp)
//   tu_mfma.hip    the pair stage on the matrix cores (pair_mfma.hpp)
//   tu_etap.hip    eta_p (eta_p.hpp)
//   tu_fused.hip   the two-launch iteration of small problems (fused_small.hpp); the triple passes with the T + S stage
//                  in one launch (pass_dense.hpp)
//   tu_once.hip    once-per-run kernels with the host side of their entries: likelihood, prod_dist / predict, omegas,
//                  the random start
//   tu_layout.hip  the layout's sorts on the device (rocPRIM)
// the serving queries, planned by serve_plan.hpp, in the frame of serve_frame.hpp; one unit per query family, one header of
// kernels per query, and every kernel launched from exactly one unit:
//   tu_serve_frame.hip the frame's out-of-line half: the kernels several families share (recommend.hpp's weights, fold,
//                      score tile, seen exclusion and selection; catalogue.hpp's compact table and exclusions by column)
//   tu_recommend.hip  the recommend session and its plain queries: recommend.hpp (top-N, positions), catalogue.hpp (within
//                     a part of the catalogue, ranking), quota.hpp (capped categories), shelves.hpp (category level)
//   tu_rerank.hip     queries with a stage of their own: explore.hpp (randomised top-N), ensemble.hpp (how far the
//                     restarts agree), group.hpp (group queries), diverse.hpp (the diversified top-N, pair distances)
//   tu_pairs.hip      top_pairs.hpp (the m best pairs), pairs_bulk.hpp (beyond 1,024, planned by pairs_bulk_plan.hpp)
//   tu_market.hip     the item side and capacity: audience.hpp (item-side queries), allocate.hpp (capacity-aware
//                     allocation), assign.hpp (welfare-maximising assignment), assortment.hpp (greedy assortment)
//   tu_similar.hip    the other sessions: similar.hpp (nearest items / users), inform.hpp (the most informative items of a
//                     user), overlap.hpp (the overlap of the restarts' groups)
//   tu_pairs_bulk.hip the device sorts of pairs_bulk.hpp and assign.hpp (rocPRIM)
//   tu_fold_in.hip    fold new users into a fitted model (fold_in.hpp)
//   tu_heldout.hip    held-out log-likelihood of every restart slot (heldout.hpp)
//   tu_explain.hip    which of a user's training rows carry a recommendation (explain.hpp)
// unity.hip includes them all into ONE unit: the diagnostic builds (-DMMSBM_STAMPS, -DMMSBM_ABLATE) and
// scripts/kernel_resources.sh use it.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/mmsbm_hip.h"
#include "layout.hpp"
#include "abi_request.hpp"
#include "common.hpp"
#include "shapes.hpp"
#include "pair_plan.hpp"
#include "step_plan.hpp"
#include "serve_plan.hpp"
#include "pairs_bulk_plan.hpp"
#include "stamps.hpp"
#include "rowtab.hpp"
#include "context.hpp"
#include "launch.hpp"
