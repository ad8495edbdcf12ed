// abi_assemble.hpp — host code shared by abi_layouts.hip and abi_frontend.hip (no kernels): how the handle adopts pose-major scans
// that are already in its device arrays, whoever put them there (clc_store_observations: copied from the host;
// clc_assemble_observations: built on the device).
#pragma once
#include "clc_abi_internal.hpp"

namespace clc_abi {

// reference-size stored scans: the host keeps the tag poses and the z flags and plans a selection's layouts itself
inline bool store_is_reference_size(size_t P, size_t M, size_t ML) { return P > 0 && P <= 4096 && M <= 16384 && ML <= 16384; }

// what the host has to know about reference-size scans (ignored for larger ones)
struct StoreFacts {
  const double* tag_q = nullptr;  // [P * 4] (w, x, y, z)
  const double* tag_t = nullptr;  // [P * 3]
  bool any_z_pts = false, any_z_ptl = false, any_z_ends = false;
  bool lines_equal_points = false;
};

// The tail of every store: h->s_pts_off / h->s_ptl_off hold the relative CSR offsets [n_poses + 1] and the copies / kernels that
// fill d_sq, d_st, d_spts, d_sptl, d_soff are enqueued on the handle's stream.  Records the facts, waits for the stream, makes the
// scans the stored ones and bumps store_generation.  (abi_layouts.hip)
int adopt_store(clc_handle* h, int n_poses, const StoreFacts& f);

}  // namespace clc_abi
