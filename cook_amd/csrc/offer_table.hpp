// offer_table.hpp — the staged offer table: its columns as a set of pointers (OfferCols) and as a set of device
// buffers (OfferStore), its widths (OfferDims), and THE list of its columns (offer_columns), which names every column once and is what
// every host flow that stages, carries, churns or fetches the table walks.  A new column is a member of OfferColsOf, a member of MatchIn
// and one line of offer_columns.  Included by engine.hip inside its anonymous namespace behind device_buf.hpp (the engine holds an
// OfferStore), and by churn_kernels.hpp (the gather's argument block holds three OfferCols); expects match_kernels.hpp (MatchIn) and
// cookmatch.h (cook_offers, cook_offer_rows).
#pragma once
#include <type_traits>

#include "fold_kernels.hpp"  // (the fold's argument structs, filled from a column set at the end of this file)

// ---- the column set ------------------------------------------------------------------------------------------------------------------------
// every column of an offer table ([rows] each; gpu_* [rows][gpu_slots], disk_* [rows][disk_slots], attr [rows][n_attr]), as P<element>
template <template <class> class P>
struct OfferColsOf {
  P<double> cpus, mem, run_cpus, run_mem, scal[3], gpu_count, disk_space;
  P<uint32_t> host, gpu_model, disk_type, attr, location;
  P<uint8_t> k8s;
  P<int32_t> max_tasks, num_tasks, run_count, ports;
  P<int64_t> host_start;
};
template <bool W>
struct OfferPtr {
  template <class T>
  using P = std::conditional_t<W, T*, const T*>;
};
// the columns as device pointers; null: the table has no such column.  W: a set that is written
template <bool W>
using OfferCols = OfferColsOf<OfferPtr<W>::template P>;

// ---- the dimensions ------------------------------------------------------------------------------------------------------------------------
enum OfferWidth : unsigned { OFFER_W_ONE, OFFER_W_GPU, OFFER_W_DISK, OFFER_W_ATTR };  // one value per row / per entry of the gpu map / of the disk map / per attribute key
struct OfferDims {
  unsigned gpu_slots, disk_slots, n_attr;  // (the slots: >= 1)
  __host__ __device__ constexpr unsigned width(OfferWidth k) const {
    return k == OFFER_W_GPU ? gpu_slots : k == OFFER_W_DISK ? disk_slots : k == OFFER_W_ATTR ? n_attr : 1u;
  }
};
static inline OfferDims offer_dims(const MatchIn& in) { return OfferDims{in.gpu_slots ? in.gpu_slots : 1u, in.disk_slots ? in.disk_slots : 1u, in.n_attr}; }

// ---- THE list ------------------------------------------------------------------------------------------------------------------------------
// what the host flows treat differently from column to column
enum : unsigned {
  OFFER_REQUIRED = 1u,  // every table has it (cpus, mem, host)
  OFFER_MADE = 2u,      // a carry or a release brings it into existence when the staged table lacks it (absent, it reads as 0 for every row)
  OFFER_FOLDED = 4u,    // a fold writes it (CarryOfferCols)
};
// one column: where it is in a column set (col: OfferCols, OfferStore), in MatchIn (in), in cook_offers (pub) and in cook_offer_rows
// (row); its width; what a NULL column means for every row (the loads of match_kernels.hpp).  The named scalars are `scalars` of the
// public structs, ONE pointer to n_scalars columns of n doubles: sub = which one
template <class T, class Col, class In>
struct OfferColumn {
  Col col;
  In in;
  const T* cook_offers::*pub;
  T* cook_offer_rows::*row;
  OfferWidth kind;
  T none;
  unsigned flags, sub;
  bool scalar;
  template <class Ptr>
  Ptr part(Ptr p, unsigned n_scalars, size_t n) const { return !scalar ? p : (p && sub < n_scalars) ? p + (size_t)sub * n : nullptr; }
  // the column on the HOST, in a caller's struct (null: not given)
  const T* of(const cook_offers& o) const { return part(o.*pub, o.n_scalars, o.n); }
  T* of(const cook_offer_rows& o) const { return part(o.*row, o.n_scalars, o.n); }
};
template <class T, class Col, class In>
__host__ __device__ constexpr OfferColumn<T, Col, In> offer_column(Col col, In in, const T* cook_offers::*pub, T* cook_offer_rows::*row, OfferWidth kind,
                                                                   std::enable_if_t<true, T> none, unsigned flags = 0u, unsigned sub = 0u, bool scalar = false) {
  return OfferColumn<T, Col, In>{col, in, pub, row, kind, none, flags, sub, scalar};
}
#define OFFER_MEMBER(m) [](auto& x) -> auto& { return x.m; }
// f(column) for every column, in the order a table is staged in (the uploads of match_stage_offers, the block of cook_cycle_update)
template <class F>
__host__ __device__ constexpr void offer_columns(F&& f) {
  using O = cook_offers;
  using R = cook_offer_rows;
  constexpr unsigned req = OFFER_REQUIRED, made = OFFER_MADE | OFFER_FOLDED, fold = OFFER_FOLDED;
  f(offer_column(OFFER_MEMBER(cpus), OFFER_MEMBER(o_cpus), &O::cpus, &R::cpus, OFFER_W_ONE, 0.0, req | fold));
  f(offer_column(OFFER_MEMBER(mem), OFFER_MEMBER(o_mem), &O::mem, &R::mem, OFFER_W_ONE, 0.0, req | fold));
  f(offer_column(OFFER_MEMBER(host), OFFER_MEMBER(o_host), &O::host, &R::host, OFFER_W_ONE, 0, req));
  f(offer_column(OFFER_MEMBER(k8s), OFFER_MEMBER(o_k8s), &O::k8s, &R::k8s, OFFER_W_ONE, 0));
  f(offer_column(OFFER_MEMBER(gpu_model), OFFER_MEMBER(o_gpu_model), &O::gpu_model, &R::gpu_model, OFFER_W_GPU, 0));
  f(offer_column(OFFER_MEMBER(gpu_count), OFFER_MEMBER(o_gpu_count), &O::gpu_count, &R::gpu_count, OFFER_W_GPU, 0.0, fold));
  f(offer_column(OFFER_MEMBER(disk_type), OFFER_MEMBER(o_disk_type), &O::disk_type, &R::disk_type, OFFER_W_DISK, 0));
  f(offer_column(OFFER_MEMBER(disk_space), OFFER_MEMBER(o_disk_space), &O::disk_space, &R::disk_space, OFFER_W_DISK, 0.0, fold));
  f(offer_column(OFFER_MEMBER(ports), OFFER_MEMBER(o_ports), &O::ports, &R::ports, OFFER_W_ONE, 0, made));
  for (unsigned s = 0; s < 3u; ++s)
    f(offer_column([s](auto& x) -> auto& { return x.scal[s]; }, [s](auto& x) -> auto& { return x.o_scal[s]; }, &O::scalars, &R::scalars, OFFER_W_ONE,
                   0.0, fold, s, true));
  f(offer_column(OFFER_MEMBER(attr), OFFER_MEMBER(o_attr), &O::attr, &R::attr, OFFER_W_ATTR, 0));
  f(offer_column(OFFER_MEMBER(max_tasks), OFFER_MEMBER(o_max_tasks), &O::max_tasks, &R::max_tasks, OFFER_W_ONE, -1));  // (no limit)
  f(offer_column(OFFER_MEMBER(num_tasks), OFFER_MEMBER(o_num_tasks), &O::num_tasks, &R::num_tasks, OFFER_W_ONE, 0, made));
  f(offer_column(OFFER_MEMBER(location), OFFER_MEMBER(o_location), &O::location, &R::location, OFFER_W_ONE, 0));
  f(offer_column(OFFER_MEMBER(host_start), OFFER_MEMBER(o_host_start), &O::host_start_s, &R::host_start_s, OFFER_W_ONE, -1));  // (absent)
  f(offer_column(OFFER_MEMBER(run_cpus), OFFER_MEMBER(o_run_cpus), &O::run_cpus, &R::run_cpus, OFFER_W_ONE, 0.0, made));
  f(offer_column(OFFER_MEMBER(run_mem), OFFER_MEMBER(o_run_mem), &O::run_mem, &R::run_mem, OFFER_W_ONE, 0.0, made));
  f(offer_column(OFFER_MEMBER(run_count), OFFER_MEMBER(o_run_count), &O::run_count, &R::run_count, OFFER_W_ONE, 0, made));
}
#undef OFFER_MEMBER
constexpr unsigned offer_column_count() {
  unsigned n = 0;
  offer_columns([&n](const auto&) { ++n; });
  return n;
}
static_assert(offer_column_count() == sizeof(OfferCols<false>) / sizeof(void*), "offer_columns visits every member of OfferColsOf once");
static_assert(COOK_MAX_SCALARS == 3, "the named scalars' columns: scal[3], o_scal[3]");

// ---- MatchIn and the list --------------------------------------------------------------------------------------------------------------------
// the staged table as a column set (a column of width 0 — attributes without keys — is none)
static inline OfferCols<false> offer_cols_of(const MatchIn& in) {
  OfferCols<false> c{};
  const OfferDims d = offer_dims(in);
  offer_columns([&](const auto& col) { col.col(c) = d.width(col.kind) ? col.in(in) : nullptr; });
  return c;
}
// `c` is the staged table from here on.  only_held: c is the part of the table a fold has written; the columns it does not hold (and
// the row count and the widths: the same rows) stay as they are
template <class Cols>  // (OfferCols<false> or <true>)
static inline void offer_cols_stage(MatchIn& in, const Cols& c, const OfferDims& d, unsigned M, bool only_held = false) {
  if (!only_held) in.M = M, in.gpu_slots = d.gpu_slots, in.disk_slots = d.disk_slots, in.n_attr = d.n_attr;
  offer_columns([&](const auto& col) { col.in(in) = (!only_held || col.col(c)) ? col.col(c) : col.in(in); });
}

// ---- the store -------------------------------------------------------------------------------------------------------------------------------
// one grow-only device buffer per column (an empty one costs nothing: a flow that writes twelve of the columns holds the same type)
struct OfferStore : OfferColsOf<DArr> {
  // room for `rows` rows in the columns `which(column)` says yes to -> those columns (the others: null)
  template <class Which>
  OfferCols<true> ensure(const OfferDims& d, size_t rows, Which&& which) {
    OfferCols<true> c{};
    offer_columns([&](const auto& col) { col.col(c) = which(col) ? col.col(*this).ensure(rows * d.width(col.kind)) : nullptr; });
    return c;
  }
};

// ---- the fold's view (fold_kernels.hpp) --------------------------------------------------------------------------------------------------------
// what fold_offers reads: the staged columns ...
static inline CarryOfferIn fold_offer_in(const OfferCols<false>& s, const OfferDims& d) {
  CarryOfferIn ci{};
  ci.cpus = s.cpus, ci.mem = s.mem, ci.run_cpus = s.run_cpus, ci.run_mem = s.run_mem, ci.gpu_count = s.gpu_count, ci.disk_space = s.disk_space;
  ci.run_count = s.run_count, ci.num_tasks = s.num_tasks, ci.ports = s.ports;
  ci.k8s = s.k8s, ci.gpu_model = s.gpu_model, ci.disk_type = s.disk_type;
  for (unsigned x = 0; x < 3u; ++x) ci.scal[x] = s.scal[x];
  ci.gpu_slots = d.gpu_slots, ci.disk_slots = d.disk_slots;
  return ci;
}
// ... and what it writes: the OFFER_FOLDED columns of a set
static inline CarryOfferCols fold_offer_cols(const OfferCols<true>& w) {
  CarryOfferCols co{};
  co.cpus = w.cpus, co.mem = w.mem, co.run_cpus = w.run_cpus, co.run_mem = w.run_mem, co.gpu_count = w.gpu_count, co.disk_space = w.disk_space;
  co.run_count = w.run_count, co.num_tasks = w.num_tasks, co.ports = w.ports;
  for (unsigned x = 0; x < 3u; ++x) co.scal[x] = w.scal[x];
  return co;
}
