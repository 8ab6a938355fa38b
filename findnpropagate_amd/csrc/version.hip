// Library identification for the ctypes loader (findnpropagate_amd/lib.py).
#include "common.h"

#define FNP_ABI_VERSION 14   // 14: fnp_assemble_sweeps_window, fnp_rows_in_boxes + fnp_rows_in_boxes_workspace_bytes were added without a version bump (new entry points only, no existing signature changed; FNP_SWEEP_FINISHED is read by the new entry alone); 14: fnp_assemble_sweeps + fnp_assemble_sweeps_workspace_bytes were added without a version bump (new entry points only, no existing signature changed); 14: fnp_sparse_to_dense_backward was added, and fnp_sparse_to_dense / _fill take FNP_F16, without a version bump (a new entry point and a new accepted dtype, no existing signature changed); 14: fnp_prepare_points + fnp_prepare_points_workspace_bytes were added without a version bump (new entry points only, no existing signature changed); 14 (round 6): fnp_gather_counts_host (the counts stored into pinned host memory by the launch itself); 13 (round 6): fnp_rankgrid.counters + fnp_rankgrid_counter_words (counted marks: the rank prefix is one launch); 12 (round 5): the wide-tile entry points of ABI 10 are gone

extern "C" const char *fnp_version(void) { return "fnp-hip gfx950 abi1"; }
extern "C" int fnp_abi_version(void) { return FNP_ABI_VERSION; }
