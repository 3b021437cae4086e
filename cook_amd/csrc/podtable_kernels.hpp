// podtable_kernels.hpp — device side of the resident pod table (cook_offers_stage_pod_ids, cook_offers_update, the pod delta of
// cook_cycle_run_queue_pods*): the pod table of a Kubernetes pool stays on the device between match cycles and takes what
// changed as short lists.  A stable compaction plus an append over every pod column, and a scatter into the node columns:
// mark (through the id table) -> ONE scan -> ONE gather of every column -> the append -> the id table's scatter -> the node rows' scatter.
//
// Index spaces: r = row of the OLD pod table (n_old rows); d = row of the NEW one; t = entry of a list (remove_id, add, node_row);
//               id = a pod's caller-chosen slot number (< id_cap); id2row[id] = r, or COOK_NONE_U32 for an id that is not live.
// The order rule: old rows keep their relative order (the scan), added rows go behind the last survivor in list order (the append
// starts at n_keep, which the host knows from its bitmap of the live ids before the first launch).
#pragma once
#include "common.hpp"
#include "multi.hpp"
#include "scan.hpp"

// one column of a table on its way through a delta: esize bytes per cell, `width` cells per row
struct PodCol {
  const void* src;          // the resident column (old rows); the node rows' scatter does not read it
  void* dst;                // where the new rows go: the column's second buffer (pods), the resident column itself (node rows)
  const void* add;          // the list's rows on the device, or null: dflt
  unsigned long long dflt;  // bit pattern of what a NULL column means
  unsigned esize, width;
};
constexpr unsigned POD_MAX_COLS = 9;  // pods: node, cpus, mem, gpus, gpu_model, disk, disk_type, flags, id; nodes: host ... flags, attr
struct PodColSet {
  PodCol c[POD_MAX_COLS];
  unsigned n_cols;
};

static __device__ __forceinline__ void pod_copy_cell(void* dst, size_t di, const void* src, size_t si, unsigned esize) {
  if (esize == 8) ((uint64_t*)dst)[di] = ((const uint64_t*)src)[si];
  else if (esize == 4) ((uint32_t*)dst)[di] = ((const uint32_t*)src)[si];
  else ((uint8_t*)dst)[di] = ((const uint8_t*)src)[si];
}
static __device__ __forceinline__ void pod_store_cell(void* dst, size_t di, unsigned long long v, unsigned esize) {
  if (esize == 8) ((uint64_t*)dst)[di] = v;
  else if (esize == 4) ((uint32_t*)dst)[di] = (uint32_t)v;
  else ((uint8_t*)dst)[di] = (uint8_t)v;
}

// keep[] is 1 beforehand.  Entry t of the remove list clears its row's keep and its id's entry of the id table; an id that is not
// live has no row (the host has counted it from its bitmap).  The host refuses ids >= id_cap and an id twice: no two entries share a row.
COOK_KERNEL void pod_mark(const uint32_t* __restrict__ remove_id, unsigned n_remove, unsigned id_cap, uint32_t* __restrict__ id2row, unsigned n_old,
                          uint8_t* __restrict__ keep) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_remove) return;
  const uint32_t id = remove_id[t];
  if (id >= id_cap) return;
  const uint32_t r = id2row[id];
  if (r < n_old) keep[r] = 0;
  id2row[id] = 0xFFFFFFFFu;
}
struct LoadPodKeep {  // 1 for a row that stays
  const uint8_t* keep;
  __device__ __forceinline__ SumI operator()(unsigned r) const { return SumI{keep[r] ? 1 : 0}; }
};

// One thread per OLD row: a row that stays moves, with every column, to (rows that stay in front of it) of the second buffers.
COOK_KERNEL void pod_gather(PodColSet cs, const uint8_t* __restrict__ keep, const SumI* __restrict__ incl, unsigned n_old, unsigned n_new) {
  const unsigned r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_old || !keep[r]) return;
  const unsigned d = (unsigned)incl[r].v - 1u;
  if (d >= n_new) return;
  for (unsigned k = 0; k < cs.n_cols; ++k) pod_copy_cell(cs.c[k].dst, d, cs.c[k].src, r, cs.c[k].esize);
}

// One thread per ADDED row: list entry t becomes row n_keep + t; a column the list lacks gives what NULL means.
COOK_KERNEL void pod_append(PodColSet cs, unsigned n_keep, unsigned n_add, unsigned n_new) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_add || n_keep + t >= n_new) return;
  const size_t d = (size_t)n_keep + t;
  for (unsigned k = 0; k < cs.n_cols; ++k) {
    if (cs.c[k].add) pod_copy_cell(cs.c[k].dst, d, cs.c[k].add, t, cs.c[k].esize);
    else pod_store_cell(cs.c[k].dst, d, cs.c[k].dflt, cs.c[k].esize);
  }
}

// id2row[id of row d] = d for every row of the table (the removed ids' entries were cleared by pod_mark; a staged table: all were)
COOK_KERNEL void pod_id_scatter(const uint32_t* __restrict__ pod_id, unsigned n, unsigned id_cap, uint32_t* __restrict__ id2row) {
  const unsigned d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= n) return;
  const uint32_t id = pod_id[d];
  if (id < id_cap) id2row[id] = d;
}

// One thread per listed node row: every node column of the table takes the list's value (or what NULL means) at node_row[t], in place;
// a column of `width` cells per row (the label rows) moves all of them.  The host refuses a row out of range or listed twice.
COOK_KERNEL void pod_node_scatter(PodColSet cs, const uint32_t* __restrict__ node_row, unsigned n_rows, unsigned n_nodes) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_rows) return;
  const uint32_t r = node_row[t];
  if (r >= n_nodes) return;
  for (unsigned k = 0; k < cs.n_cols; ++k) {
    const unsigned w = cs.c[k].width;
    for (unsigned x = 0; x < w; ++x) {
      if (cs.c[k].add) pod_copy_cell(cs.c[k].dst, (size_t)r * w + x, cs.c[k].add, (size_t)t * w + x, cs.c[k].esize);
      else pod_store_cell(cs.c[k].dst, (size_t)r * w + x, cs.c[k].dflt, cs.c[k].esize);
    }
  }
}
