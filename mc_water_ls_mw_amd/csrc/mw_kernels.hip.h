// mw_kernels.hip.h -- gfx950 (MI355X, CDNA4) device code of the mW energy engine.
//
// What each kernel stands behind in the reference (keb721/mc_water_ls_mw):
//   k_build_neighbours  compute_neighbours       molint.F90:501-559
//   k_model_energy      compute_model_energy     molint.F90:407-499
//   k_move_energy / k_local_energy_single   compute_local_real_energy molint.F90:220-404
//   k_model_forces      (no counterpart: the gradient of compute_model_energy, forces and virial)
//   k_ice_q / k_ice_class  (no counterpart: CHILL+ ice structure classes of every molecule)
//   k_rdf_tiles / k_rdf_small  (no counterpart: pair-distance histogram of every box, all pairs and periodic images)
//   k_ice_clusters      (no counterpart: connected clusters of the molecules of selected CHILL+ classes)
// None of it is a translation: the list is slot-major and packed for coalesced
// reads, positions of a whole box are staged in LDS, the three-body sum is
// evaluated from per-atom moments in O(neighbours), and the single-move path
// maps one request onto one 64-wide wavefront.  Double precision throughout;
// this is gather + transcendental work, so no MFMA.
//
// The device code lives in nine headers, included here in dependency order:
//   mw_common.hip.h       constants, packed list entry, fp64 primitives, wave/DPP reductions
//   mw_neighbours.hip.h   neighbour-list builders
//   mw_full_energy.hip.h  full-box energy
//   mw_move_energy.hip.h  local energy / fused trial-move energy: k_move_energy, k_move_fallback, k_local_energy_single; includes
//                         mw_local_energy (the plain routines), mw_move_scan (the fused scan), mw_move_moments (the moment path)
//                         and mw_local_server.hip.h (the resident mailbox server)
//   mw_sweep.hip.h        device-resident Monte Carlo driver (k_sweep; includes mw_sweep_common / _volume / _decide.hip.h)
//   mw_forces.hip.h       forces and virial of the full-box energy
//   mw_ice.hip.h          per-molecule ice structure classes (CHILL+)
//   mw_rdf.hip.h          pair-distance histograms for g(r) and n(r)
//   mw_ice_clusters.hip.h clusters of ice-like molecules (largest cluster, cluster sizes)
#pragma once

#include "mw_common.hip.h"
#include "mw_neighbours.hip.h"
#include "mw_full_energy.hip.h"
#include "mw_move_energy.hip.h"
#include "mw_sweep.hip.h"
#include "mw_forces.hip.h"
#include "mw_ice.hip.h"
#include "mw_rdf.hip.h"
#include "mw_ice_clusters.hip.h"
