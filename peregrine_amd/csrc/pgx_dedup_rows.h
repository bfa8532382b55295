// pgx_dedup_rows.h -- what pgx_dedup.hip shares with the stages that read a graph-mode stream's rows in HBM (pgx_sgraph.hip): the row
// and the stream.  (The pieces of a text line and the staging that device text leaves through: pgx_text.h.)
#pragma once
#include "pgx_text.h"

namespace pgx {
// a line of the dedup text before it is printed (shmr_dedup.c:44-89: the coordinates already transformed)
struct Row {
  uint32_t rid0, rid1;
  int32_t m_size, dist;
  uint32_t a_bgn, a_end, rlen0, strand, b_bgn, b_end, rlen1, type;
};

// the three IEEE double operations of shmr_dedup.c:89-90 in that order, never contracted
__device__ inline double err_est_of(int32_t dist, int32_t m_size) {
#pragma clang fp contract(off)
  const double p = 100.0 * (double)dist;
  const double q = p / (double)m_size;
  return 100.0 - q;
}

}  // namespace pgx

struct pgx_dedup_stream {
  pgx::DevBuf<unsigned long long> tab;   // the seen-pair set: cap slots + the word of the all-ones key; owned by the stream (MemTag "dedup")
  uint64_t cap = 0;
  uint64_t n_records = 0, n_unique = 0;
  bool failed = false;              // an entry point returned an error: only pgx_dedup_close is accepted
  bool shut = false;                // pgx_shutdown ran while the stream was open: its device state is gone
  pgx::TextStage stage;             // text staging (pinned), made at the first feed that has text
  // graph mode (pgx_dedup_open_graph): the lines wait in HBM as rows until the end of the stream says which reads are contained
  bool graph = false;
  bool draining = false;            // the first pgx_dedup_drain ran: the store holds exactly the kept lines' rows, no feed is accepted
  pgx::DevBuf<uint32_t> bits;            // contained reads, one bit per read id (MemTag "dedup"); bits.n words, a power of two
  pgx::DevBuf<pgx::Row> store;           // rows of the `overlap` lines between two unmarked reads, in stream order; store.n is the capacity
  uint64_t store_n = 0, drained = 0;   // rows held; rows handed out as text
  bool released = false;            // the last line was handed out and the store went back: nothing left for pgx_sgraph_build
  void drop_device_state() {
    tab.release();
    bits.release(), store.release();
    stage.drop();
  }
};

namespace pgx {
// the end of a graph-mode stream: the store compacted against the final bitmap (sets s->draining; from then on feeds are refused)
void graph_compact(pgx_dedup_stream *s);
// a live graph's edge records on the device, in creation order with their final types (pgx_sgraph.hip; `who` names the caller in the
// error a freed context gives); what reads them runs on ctx().stream, behind the build
const pgx_sgraph_edge *sgraph_device_edges(const pgx_sgraph *g, const char *who, uint64_t *n);
// live unitigs' arrays on the device (pgx_unitigs.hip): the table, the path array (creation indices, unitig after unitig) and, per path
// slot, its unitig and the key of the node its edge enters.  Nothing is copied: the view holds while the unitigs live.
struct UnitigsView {
  const pgx_unitig *tab;
  const uint32_t *paths, *slot_u;
  const uint64_t *slot_w;
  uint64_t n_u, m;
  uint64_t serial;   // which unitigs these are: never given twice, whatever address a later object gets
};
UnitigsView unitigs_device_view(const pgx_unitigs *u, const char *who);
bool unitigs_live(const pgx_unitigs *u, uint64_t serial);   // the unitigs of that serial: handed out by a builder, not freed, no pgx_shutdown since
}  // namespace pgx
