/*
 * pgx.h -- C-ABI of libpgx.so: the MI355X (gfx950) implementation of Peregrine's SHIMMER index + overlap
 * hot path.  Plain pointers and sizes only; no torch / C++ types.  Every entry point returns 0 on success
 * or a negative PGX_E* code (the reference exit(1)s / asserts instead: shmr_index.c:15-19,111-114,
 * shmr_utils.c:101-104); pgx_last_error() gives the message.  One context per process, one process per GPU.
 *
 * What each group replaces in the reference (/root/reference):
 *   stage level    : main() of src/shmr_index.c:37-245 and src/shmr_overlap.c:233-419 (the two executables that
 *                    py/scripts/pg_run.py:232-244,305-317 runs per chunk)
 *   resident level : the same stages with the seqdb already in HBM (what bench.py times)
 *   batch level    : mm_sketch (src/mm_sketch.c:70-151), mm_reduce (src/shmr_reduce.c:53-90), mm_count
 *                    (src/shmr_utils.c:131-160), ovlp_match (src/DWmatch.c:66-204) over many reads / pairs
 *   shimmer4py     : the cdef surface of py/peregrine/build_shimmer4py.py:8-84 (same symbol names and C
 *                    signatures) so a ctypes / cffi-ABI loader can stand in for peregrine._shimmer4py
 */
#ifndef PGX_H
#define PGX_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PGX_OK 0
#define PGX_EARG -1    /* bad argument (the reference would assert) */
#define PGX_EIO -2     /* file open/read/write failure (the reference would exit(1)) */
#define PGX_EHIP -3    /* HIP runtime error / no device */
#define PGX_ENOMEM -4
#define PGX_ESTATE -5  /* pgx_init not called; or the call needs something the state no longer has (the seqdb bytes after pgx_seqdb_release_bytes / pgx_seqdb_compact_bytes) */
#define PGX_EINVAL -6  /* the input holds, or the call asks for, something this library refuses to approximate (pgx_sgraph_build) */

/* ---- types shared with the on-disk formats (src/shimmer.h:24-30,61-64,97-110) ---- */
typedef struct { uint64_t x, y; } pgx_mm128;                        /* x = hash<<8|span ; y = rid<<32|lastPos<<1|strand */
typedef struct { uint64_t mer; uint32_t count; uint32_t pad; } pgx_mm_count;
typedef struct { int32_t m_size, dist, q_bgn, q_end, t_bgn, t_end, t_m_end, q_m_end; } pgx_match;
typedef struct {
  uint64_t y0, y1;
  uint32_t rl0, rl1;
  uint8_t strand0, strand1, ovlp_type, pad0;
  pgx_match match;
  uint32_t pad1;
} pgx_ovlp; /* 64 bytes; pad0/pad1 are written as 0 */

/* one candidate alignment: query = read rid0 from byte q_off on strand dir0, target = whole read rid1 on dir1
 * (the arguments shimmer_to_overlap passes to ovlp_match, src/shmr_overlap.c:117-125) */
typedef struct { uint32_t rid0, rid1, q_off; uint8_t dir0, dir1, pad[2]; } pgx_align_key;

/* one shimmer-pair record of build_map (src/shmr_utils.c:337-400: mp128_t {y0, y1, direction} filed under [key0][key1]) in the
 * form the ranks of a multi-GPU job exchange: npos = ~((y0 & 0xFFFFFFFF) >> 1), the descending-position sort key */
typedef struct { uint64_t key0, key1, y0; uint32_t npos; uint8_t dir, pad[3]; } pgx_pair_rec; /* 32 bytes */

typedef struct pgx_seqdb pgx_seqdb; /* opaque: a read database resident in HBM */

/* ---- context ---- */
int pgx_init(int device);            /* select the GPU, create the stream; idempotent */
void pgx_shutdown(void);
const char *pgx_last_error(void);
int pgx_device_count(void);
const char *pgx_version(void);
/* the grid a persistent kernel gets for n_items at per_cu workgroups per CU: min(n_items, CUs * per_cu), and under the test hook
 * PGX_GRID_CAP=c (read at every launch) at most c.  For tests: to see that the hook holds, and to size inputs from the device's CU count.
 * Call pgx_init first: the CU count is the selected device's (before that, the answer assumes 256 CUs). */
uint32_t pgx_stride_grid(uint64_t n_items, uint32_t per_cu);
void pgx_free(void *p);              /* releases any host array returned by this library */

/* per-kernel device time (HIP events on the library's stream), accumulated since the last reset.
 * names: "sketch", "sketch_general", "sketch_redo", "sketch_nreads", "sketch_gather", "pack", "reduce", "count", "pairs", "replay_dense" / "replay_rows" / "replay_update" (k_eval, k_eval_rows, k_update of the device replay; only with PGX_REPLAY_TIMING=1), "align" (k_align_ph), "align1" (k_align1: launches of
 * at most 13 k alignments), "align1t" (k_align1t: alignments with a target offset), "tile_geom", "stitch" (the contig layout), "encode", "dedup", "map", "sgraph" (the string graph: build and text; its parts also as "sgraph_edges", "sgraph_adj", "sgraph_tr", "sgraph_chimer", "sgraph_spur",
 * "sgraph_best", "sgraph_text"), "unitigs" (its parts: "unitigs_links", "unitigs_rank", "unitigs_paths", "unitigs_text"), "ctg_paths" (its parts:
 * "ctg_paths_graph", "ctg_paths_clean", "ctg_paths_walk", "ctg_paths_text"), "gfa" (the build with the layout of the segments; its own parts:
 * "gfa_dual", "gfa_rows", "gfa_links", "gfa_text"). */
int pgx_timing_get(const char *kernel, double *total_ms, uint64_t *launches, uint64_t *units);
void pgx_timing_reset(void);
/* HBM ledger: JSON text of the library's device memory -- live bytes, bytes held in the block cache, and the live bytes BY OWNER (seqdb,
 * packs, index workspaces, join tables, replay tables ...) at the moment the live total peaked; the named workspaces; what the driver
 * reports as used.  Returns the length of the text (buf may be NULL to ask for it).  reset_peak != 0: the peak starts again from now. */
int pgx_mem_ledger(char *buf, size_t cap, int reset_peak);

/* ---- resident read database ---- */
/* rid/rlen/roff: the idx file's columns in file order (src/shmr_mkseqdb.c:111-112); copies to HBM. */
int pgx_seqdb_upload(const uint8_t *seqdb, size_t nbytes, const uint32_t *rid, const uint32_t *rlen,
                     const uint64_t *roff, uint32_t nreads, pgx_seqdb **out);
int pgx_seqdb_load(const char *seqdb_prefix, pgx_seqdb **out); /* reads <prefix>.idx + <prefix>.seqdb */
/* the same with the seqdb bytes already in HBM (e.g. all-gathered over xGMI by the ranks of a multi-GPU job): d_seqdb is a
 * device pointer, copied device-to-device; rid/rlen/roff are host arrays */
int pgx_seqdb_upload_dev(const uint8_t *d_seqdb, size_t nbytes, const uint32_t *rid, const uint32_t *rlen,
                         const uint64_t *roff, uint32_t nreads, pgx_seqdb **out);
/* the same WITHOUT a copy: the library reads the bytes where they are (d_seqdb stays owned by the caller and must outlive the
 * pgx_seqdb).  capacity >= nbytes + 1024: the library zeroes [nbytes, nbytes + 1024) once (its kernels' wide loads may run
 * that far past the last read).  This is what lets the ranks of a multi-GPU job all-gather the job's read set straight into
 * its final place -- one copy of the seqdb per GPU instead of three (93 GB at 30x human). */
int pgx_seqdb_adopt_dev(uint8_t *d_seqdb, size_t nbytes, size_t capacity, const uint32_t *rid, const uint32_t *rlen,
                        const uint64_t *roff, uint32_t nreads, pgx_seqdb **out);
void pgx_seqdb_free(pgx_seqdb *db);
/* The seqdb's BYTES out of HBM once the 2-bit packs exist (a quarter of the size, the same information; built by the first overlap stage on
 * the database, or here): the index stage's closed-form kernels and every alignment kernel of the default path read the packs.  Refused --
 * PGX_ESTATE, bytes kept -- for a database with a read that holds an ambiguous base (sketched run by run / aligned nibble by nibble from the
 * bytes: src/mm_sketch.c:112-113, src/DWmatch.c:136-137) or a read longer than 65,535 bases.  Afterwards the entry points that need bytes (w / k
 * other than 80 / 16, want_l0, PGX_INDEX_HPC, pgx_sketch_batch) return PGX_ESTATE; a buffer handed over with pgx_seqdb_adopt_dev is no longer referenced.
 * A database with ambiguous bases gives its bytes back through pgx_seqdb_compact_bytes instead. */
int pgx_seqdb_release_bytes(pgx_seqdb *db);
int pgx_seqdb_has_bytes(const pgx_seqdb *db);
/* The same for a database WITH ambiguous bases: the packs are built if need be, the bytes of the flagged reads alone (those that hold a byte without
 * a 2-bit code) are copied into a side store, and the whole-seqdb bytes go (an adopted buffer is no longer referenced).  The packs then serve
 * every kernel of the default path; a candidate alignment that touches a flagged read, and the run-by-run sketch of a flagged read, run the
 * byte-wise kernels on the side store plus their unflagged partners' bytes, rebuilt from the packs for that call -- results stay bit-exact.
 * Without a flagged read it is pgx_seqdb_release_bytes.  Idempotent.  PGX_ESTATE, bytes kept, nothing changed: a read longer than 65,535
 * bases, packs that cannot be built, or bytes that are gone already without a side store.  Afterwards pgx_seqdb_has_bytes answers 0 and what
 * needs the whole bytes (w / k other than 80 / 16, want_l0, pgx_sketch_batch) answers PGX_ESTATE as after a release. */
int pgx_seqdb_compact_bytes(pgx_seqdb *db);
/* HBM the side store of a compacted database holds (at most length + 64 bytes per flagged read, + 4 KiB); 0 before compaction and for a
 * database without flagged reads. */
uint64_t pgx_seqdb_side_bytes(const pgx_seqdb *db);
/* One read's biseq bytes (rlen[rid] of them, cap >= that) as the seqdb file holds them, to host memory, in whatever state the database is:
 * from the bytes, or -- compacted -- from the side store / rebuilt from the packs.  After pgx_seqdb_release_bytes: PGX_ESTATE. */
int pgx_seqdb_read_bytes(pgx_seqdb *db, uint32_t rid, uint8_t *out, size_t cap);
uint64_t pgx_seqdb_bases(const pgx_seqdb *db);
uint32_t pgx_seqdb_reads(const pgx_seqdb *db);

/* ---- index stage (replaces shmr_index) ---- */
typedef struct {
  int total_chunk;   /* -t */
  int mychunk;       /* -c, 1-based; selects reads with rid % t == c % t (shmr_index.c:157) */
  int levels;        /* -l 1|2 */
  int reduction;     /* -r (<256) */
  int window;        /* -w (24..255) */
  int kmer;          /* -k (12..28) */
  int want_l0;       /* -m : also return / write the L0 list and its counts; | PGX_INDEX_HPC: see below */
} pgx_index_params;
/* -H : homopolymer-compressed shimmers, mm_sketch's is_hpc = 1 (src/mm_sketch.c:89-99): minimizers of the compressed read, positions and
 * spans in raw coordinates.  A flag OR-ed into want_l0 (whose own values stay 0, 1, or "another number": general path, no L0 files), so the
 * struct keeps its size and callers built against an older header need no recompile.  (A want_l0 with bit 8 set -- 256, any negative number
 * -- therefore no longer means "another number": pass 2 for that.)  With it the stage takes the general path (sketch,
 * reduce x levels, count) and reads the seqdb's bytes: PGX_ESTATE once they are released or compacted.  Files keep their names and formats. */
#define PGX_INDEX_HPC 0x100

typedef struct {
  pgx_mm128 *l0; size_t n_l0;           /* only when want_l0 */
  pgx_mm_count *l0_mc; size_t n_l0_mc;
  pgx_mm128 *top; size_t n_top;         /* L1 (levels==1) or L2 */
  pgx_mm_count *top_mc; size_t n_top_mc;/* sorted by mer (the reference writes khash slot order; consumers only aggregate) */
  uint64_t bases; uint32_t reads;       /* what this chunk sketched */
  uint32_t reads_literal;               /* reads sketched run by run (ambiguous bases, or flagged by a closed-form kernel: pgx_sketch_n.hip); the name is round 1's */
  double gpu_ms;                        /* device time of this call */
} pgx_index_result;

int pgx_index_resident(pgx_seqdb *db, const pgx_index_params *p, pgx_index_result *out);
void pgx_index_result_free(pgx_index_result *r);
/* file level: same flags, same output file names/bytes as shmr_index (MC files: same (mer,count) multiset) */
int pgx_index_chunk(const char *seqdb_prefix, const char *out_prefix, const pgx_index_params *p,
                    pgx_index_result *stats /* nullable; arrays are not returned */);

/* ---- sequence database (replaces shmr_mkseqdb, src/shmr_mkseqdb.c:99-121) ----
 * seq_dataset_path: text file with one FASTA/FASTQ(.gz) path per whitespace-separated token; writes <prefix>.seqdb and
 * <prefix>.idx byte-identical to the reference's.  The two-strand encoding runs on the GPU. */
int pgx_mkseqdb(const char *seq_dataset_path, const char *seqdb_prefix, uint64_t *n_reads, uint64_t *n_bases);
/* A FASTA text to a resident database, on the GPU (record grammar, compaction and two-strand encoding: pgx_fasta.hip).
 * text: FASTA at a host pointer (on_device == 0) or a device pointer (!= 0; what the caller's stream enqueued comes first after
 * pgx_stream_wait).  *out: a database whose rid are 0 .. n-1 in text order, bytes in place, equal in every field and byte to
 * pgx_seqdb_load of the files pgx_mkseqdb writes from the same text.  *names (pgx_free): the names, a line each, in rid order.
 * PGX_EINVAL: no record in the text; a line behind the first header's that starts with '+' (a FASTQ record: the message carries the
 * smallest such byte offset); a record of 2^32 bases or more.  PGX_ENOMEM: the text does not fit beside its database. */
int pgx_seqdb_from_fasta(const char *text, size_t len, int on_device, pgx_seqdb **out, char **names, size_t *names_len,
                         uint64_t *n_reads, uint64_t *n_bases);
/* <prefix>.seqdb / <prefix>.idx of a database whose bytes are in place (PGX_ESTATE once released or compacted), idx lines
 * "%09d %s %u %lu\n" with the names given: byte for byte shmr_mkseqdb's two files. */
int pgx_seqdb_save(pgx_seqdb *db, const char *names, size_t names_len, const char *seqdb_prefix);
/* FASTA/FASTQ texts, in pieces and from several files, to one resident database on the GPU (pgx_reads.hip): the whole
 * grammar of the reference's reader, its '+' branch included.  A builder is a live device object (pgx_shutdown drops its device state;
 * its calls then answer PGX_ESTATE; close it).
 * open:   room for reserve_bases bases is set aside (the store grows by doubling when they do not suffice).
 * feed:   the next `len` bytes of the current file, at a host (on_device == 0) or device pointer; ends_file != 0: they are the file's last
 *         (len may be 0).  Records whose whole parse lies inside the bytes seen are encoded into the store, rid running on across files;
 *         the text from the first unfinished header on is kept on the device.  A record the reader calls truncated ends its FILE's
 *         records, not the call.  PGX_EINVAL: 2^31 lines in one piece and its carry, 2^32 records, a record of 2^32 bases; and an empty
 *         line inside a quality block behind a '\r' that the reader would strip from an earlier line (the message names its byte offset
 *         in the file) -- nothing else that the reference reads is refused.
 * finish: the database (as pgx_seqdb_from_fasta's: equal in every field and byte to pgx_seqdb_load of the files pgx_mkseqdb writes from
 *         the same inputs) and the names, a line each (pgx_free).  PGX_EINVAL: no record at all.  The builder is empty afterwards.
 * from_files: a list file as pgx_mkseqdb reads it (whitespace-separated paths, plain or .gz), each file inflated on the calling thread
 *         and fed in pieces of PGX_FROM_READS_PIECE bytes (default 256 MiB) from a pinned buffer.
 * read_lengths: the lengths of db's reads by rid (cap: room at rlen_by_rid, at least pgx_seqdb_reads(db)). */
typedef struct pgx_seqdb_builder pgx_seqdb_builder;
int pgx_seqdb_builder_open(uint64_t reserve_bases, pgx_seqdb_builder **out);
int pgx_seqdb_builder_feed(pgx_seqdb_builder *b, const char *text, size_t len, int on_device, int ends_file);
int pgx_seqdb_builder_finish(pgx_seqdb_builder *b, pgx_seqdb **out, char **names, size_t *names_len, uint64_t *n_reads,
                             uint64_t *n_bases);
void pgx_seqdb_builder_close(pgx_seqdb_builder *b);
int pgx_seqdb_from_files(const char *seq_dataset_path, pgx_seqdb **out, char **names, size_t *names_len, uint64_t *n_reads,
                         uint64_t *n_bases);
int pgx_seqdb_read_lengths(const pgx_seqdb *db, uint32_t *rlen_by_rid, size_t cap);

/* ---- overlap stage (replaces shmr_overlap) ---- */
typedef struct {
  int total_chunk, mychunk;  /* -t -c : bucket ownership (x>>8) % t == c % t (shmr_utils.c:337,362) */
  int bestn;                 /* -b (uint8 in the reference) */
  int mc_lower, mc_upper;    /* -m -M */
  int align_bandwidth;       /* -w */
  int ovlp_upper;            /* -n */
} pgx_overlap_params;

typedef struct {
  uint64_t n_records;        /* ovlp_t records produced */
  uint64_t n_pair_records;   /* shimmer-pair records built (build_map) */
  uint64_t n_buckets;        /* buckets processed (2 < n <= ovlp_upper) */
  uint64_t n_align_needed;   /* alignments the reference would have computed */
  uint64_t n_align_gpu;      /* alignments computed on the GPU (>= needed: speculative replay) */
  uint64_t n_seen_skip;
  uint32_t rounds;           /* replay rounds until the fixed point */
  double gpu_ms;             /* device time */
  double host_ms;            /* host orchestration time (order emulation + replay) */
  uint64_t n_evaluations;    /* bucket evaluations of the replay (>= n_buckets: the fixed point re-evaluates) */
  uint32_t device_replay;    /* 1: the greedy walk ran on the GPU (pgx_replay.hip); 0: on the host threads */
  uint32_t device_visit;     /* 0: bucket visit order built by host threads; else 1 + the number of first-key groups a whole
                                wavefront replayed (pgx_visit.hip; the others take a lane each) */
  uint32_t replay_attempts;  /* device replay: attempts until the tables were large enough (1: the first sizes held; the sizes a
                                stage needed are where the next stage of the process starts) */
  uint32_t reserved0;
  uint64_t stream_checksum;  /* order-sensitive 64-bit checksum of the records' fields (padding bytes excluded), computed where the
                                records are written: two stages with equal checksums produced the same stream (0: not computed) */
} pgx_overlap_stats;

/* mmers: concatenation of all index chunks' final-level lists in chunk order; counts: all MC entries */
int pgx_overlap_resident(pgx_seqdb *db, const pgx_mm128 *mmers, size_t n_mm, const pgx_mm_count *counts,
                         size_t n_counts, const pgx_overlap_params *p, pgx_ovlp **out, size_t *n_out,
                         pgx_overlap_stats *stats);
/* index + overlap of a single-chunk job in one call: the final-level list and its counts stay in HBM between the two
 * stages (the reference hands them over through files).  ip must name chunk 1 of 1.  want_index_arrays == 0: index_out
 * carries the sizes / statistics only (top, top_mc stay NULL).  Results are those of pgx_index_resident followed by
 * pgx_overlap_resident. */
int pgx_index_overlap_resident(pgx_seqdb *db, const pgx_index_params *ip, const pgx_overlap_params *op,
                               int want_index_arrays, pgx_index_result *index_out, pgx_ovlp **out, size_t *n_out,
                               pgx_overlap_stats *stats);
/* ---- multi-GPU hand-over, everything device-resident (one process per GPU, chunk c on rank c-1) ----
 * The reference couples the chunks through files: every overlap chunk reads EVERY index chunk's list and counts
 * (src/shmr_overlap.c:359-384) and keeps the records whose first key it owns (src/shmr_utils.c:337,362).  Here each rank
 * builds the pair records of its OWN index chunk's reads and routes them to the owner chunk: the caller moves (1) the count
 * tables with an all-gather and (2) the records with an all-to-all(v) (RCCL), both on device pointers, between these calls:
 *   pgx_index_resident_dev   : index stage; the final-level list and its counts stay in HBM (*d_top, *d_mc: library-owned, valid
 *                              until the next index call of this process)
 *   pgx_pairs_prepare_dev    : d_counts_all = all chunks' count tables concatenated; flags the kept shimmers of d_top;
 *                              *first_strict = list index of the first shimmer with lower <= count < upper, -1 if none (the global
 *                              scan starts there, src/shmr_utils.c:311-320: the caller passes `start` = that index on the first rank
 *                              that has one, 0 on later ranks, -1 on earlier ranks)
 *   pgx_pairs_scatter_dev    : *d_send = the records grouped by destination chunk 1..total_chunk, scan order inside a group
 *                              (library-owned, valid until the next prepare); send_counts[c-1] = records for chunk c
 *   pgx_overlap_records_dev  : overlap stage of chunk p->mychunk over the records received, concatenated in SOURCE chunk order
 *                              (then scan order) = the insertion order of build_map over the concatenated lists; results are
 *                              those of pgx_overlap_resident on the concatenated lists */
int pgx_index_resident_dev(pgx_seqdb *db, const pgx_index_params *p, pgx_index_result *stats, const pgx_mm128 **d_top,
                           size_t *n_top, const pgx_mm_count **d_mc, size_t *n_mc);
int pgx_pairs_prepare_dev(pgx_seqdb *db, const pgx_mm128 *d_top, size_t n_top, const pgx_mm_count *d_counts_all,
                          size_t n_counts_all, int mc_lower, int mc_upper, int64_t *first_strict);
int pgx_pairs_scatter_dev(pgx_seqdb *db, int total_chunk, int64_t start, const pgx_pair_rec **d_send, uint64_t *send_counts);
int pgx_overlap_records_dev(pgx_seqdb *db, const pgx_pair_rec *d_records, size_t n_records, const pgx_overlap_params *p,
                            pgx_ovlp **out, size_t *n_out, pgx_overlap_stats *stats);
/* overlap stage over DEVICE lists (the concatenation of all index chunks' lists / counts, e.g. after an all-gather) */
int pgx_overlap_resident_dev(pgx_seqdb *db, const pgx_mm128 *d_mmers, size_t n_mm, const pgx_mm_count *d_counts,
                             size_t n_counts, const pgx_overlap_params *p, pgx_ovlp **out, size_t *n_out,
                             pgx_overlap_stats *stats);
/* Ordering against another runtime's stream (e.g. the stream torch / RCCL enqueued a collective on) without stopping the host:
 *   pgx_stream_wait(s)   : work the library enqueues from now on starts after everything enqueued on s so far
 *   pgx_stream_signal(s) : work enqueued on s from now on starts after everything the library has enqueued so far
 * s is a hipStream_t (NULL = the default stream).  The replacement for a full stream synchronisation around each hand-over. */
int pgx_stream_wait(void *other_stream);
int pgx_stream_signal(void *other_stream);
/* plain device-to-device copy on the library's stream, synchronous (for callers that hold device memory of another runtime) */
int pgx_copy_dev(void *d_dst, const void *d_src, size_t nbytes);

/* file level: globs <shimmer_prefix>-[0-9]*-of-[0-9]*.dat and -MC- twins like shmr_overlap.c:355-384 */
int pgx_overlap_chunk(const char *seqdb_prefix, const char *shimmer_prefix, const char *out_path,
                      const pgx_overlap_params *p, pgx_overlap_stats *stats);
/* Asynchronous delivery of the overlap records (resident pipelines that run several chunks in one process).  pgx_results_async(1): the
 * pgx_overlap_*resident* entry points return once the copy of their records to the host array is ENQUEUED (on a stream of its own,
 * behind the kernel that writes them) instead of finished; *n_records, the statistics and the array's address are valid at once, the
 * array's CONTENT only after pgx_results_wait() -- which the next overlap stage, pgx_free of the array and pgx_results_async(0) also
 * imply.  Returns the previous setting.  Off by default: every call returns finished arrays. */
int pgx_results_async(int on);
int pgx_results_wait(void);

/* The same two stages on a read database that is ALREADY resident (pgx_seqdb_load / _upload): what a long-lived process serves
 * several chunk commands from -- `pgx_cli serve`, which the shmr_index / shmr_overlap drop-ins attach to, INTEGRATION.md section 5 --
 * so that a job's 8 + 8 chunk commands upload the seqdb once instead of sixteen times. */
int pgx_index_chunk_db(pgx_seqdb *db, const char *out_prefix, const pgx_index_params *p, pgx_index_result *stats);
int pgx_overlap_chunk_db(pgx_seqdb *db, const char *shimmer_prefix, const char *out_path, const pgx_overlap_params *p,
                         pgx_overlap_stats *stats);
/* The overlap command of a served JOB in two steps (round 6; caller contract py/scripts/pg_run.py:305-317 -- the job's commands follow
 * each other against one resident database).  pgx_overlap_chunk_db_begin returns when the GPU stage is done and the records are on
 * their way from the device to out_path (the statistics are final); pgx_output_finish blocks until that file is complete and closed,
 * reports an I/O error and releases *pending -- it may be called from another thread while the next command's _begin already runs,
 * which is how `pgx_cli serve` overlaps one command's file with the next command's kernels.  pgx_overlap_chunk_db = _begin + _finish.
 * An index command on a resident database leaves device copies of the list / count files it wrote; _begin assembles its lists from
 * those copies (checked against the files' size and mtime) and reads only files it holds no current copy of. */
typedef struct pgx_output pgx_output;
int pgx_overlap_chunk_db_begin(pgx_seqdb *db, const char *shimmer_prefix, const char *out_path, const pgx_overlap_params *p,
                               pgx_overlap_stats *stats, pgx_output **pending);
int pgx_output_finish(pgx_output *pending);

/* ---- dedup (replaces shmr_dedup, src/shmr_dedup.c:32-101) ----
 * recs: the concatenated ovlp_t streams (cat ovlp*.dat).  The first record of every read pair wins; *text receives the
 * FALCON-style overlap lines (malloc'd, release with pgx_free), byte-identical to the reference's stdout. */
int pgx_dedup(const pgx_ovlp *recs, size_t n, char **text, size_t *text_len, uint64_t *n_unique);
/* The same as a STREAM, for a job's worth of records in bounded memory: the concatenation of the texts of all feeds, in feed order, is byte
 * for byte what pgx_dedup returns for the concatenation of the fed records (the first record of every unordered read pair in stream order
 * wins; a feed returns the lines of the pairs first seen in that feed, in the order of their records).  The seen-pair set stays in HBM for
 * the stream's life and grows as needed -- by the pairs a feed really adds, so a stream opened with its exact number of pairs never
 * grows (expected_pairs sizes it up front; 0: start small and grow); first-wins, the coordinate
 * transform and the text lines are computed on the GPU.
 *   pgx_dedup_feed     : recs is a host array
 *   pgx_dedup_feed_dev : d_recs is a device pointer (records another runtime holds in HBM: order its stream first, pgx_stream_wait)
 * A feed takes n < 2^31 records, the stream as a whole has no limit.  *text is malloc'd (pgx_free), NUL-terminated, *text_len == 0 for a
 * feed that adds nothing or has n == 0.  A stream that returned an error accepts only pgx_dedup_close, which frees it (always) and
 * reports the records fed and the lines written.  A stream left open across pgx_shutdown loses its device state and accepts only
 * pgx_dedup_close.  PGX_DEDUP_HOST_TEXT=1 (diagnostic) prints the lines with snprintf on the host instead. */
typedef struct pgx_dedup_stream pgx_dedup_stream;
int pgx_dedup_open(uint64_t expected_pairs, pgx_dedup_stream **out);
int pgx_dedup_feed(pgx_dedup_stream *s, const pgx_ovlp *recs, size_t n, char **text, size_t *text_len);
int pgx_dedup_feed_dev(pgx_dedup_stream *s, const pgx_ovlp *d_recs, size_t n, char **text, size_t *text_len);
int pgx_dedup_close(pgx_dedup_stream *s, uint64_t *n_records, uint64_t *n_unique);
/* GRAPH MODE of the stream: only the lines the string graph's loader can use (ovlp_to_graph.py:677-770 reads every line, keeps the
 * `overlap` lines, and then skips those with a read in contained_reads).  A printed line with rid0 != rid1 marks a read contained: rid0 if
 * its type is `contained` (every ovlp_type but 0 and 1), rid1 if it is `contains`; a self pair marks nothing and a record that lost
 * first-wins prints -- and marks -- nothing.  The stream hands out, in stream order, exactly the lines of type `overlap` with
 * rid0 != rid1 and neither read marked by ANY line of the whole stream; the loader makes the same add_edge calls from them as from the full
 * text, for every --min_len / --min_idt (neither is applied here).  Read ids are compared as 32-bit numbers.
 *   pgx_dedup_open_graph : as pgx_dedup_open.  pgx_dedup_feed / _feed_dev return *text_len == 0: the lines wait in HBM as 48-byte rows
 *                          (rows whose read is marked already are not even stored), beside a bitmap of the marked reads (one bit per id up
 *                          to the largest marked one, 512 MiB at most).  No host spill: PGX_ENOMEM fails the stream.
 *   pgx_dedup_drain      : after the last feed, the kept lines in order, at most max_lines (> 0) and 2^24 per call;
 *                          *text as from a feed, *done != 0 with the last of them (at once on a stream that keeps nothing).  The
 *                          first call compacts the rows against the final bitmap; from then on feeds are refused with PGX_ESTATE (which
 *                          does not fail the stream).
 *   pgx_dedup_graph_stats: reads marked so far, lines kept (final once a drain has run; before, the rows held -- an upper bound), lines
 *                          a plain stream would have written so far (pgx_dedup_close's n_unique).  Any of the three may be NULL.
 * Both refuse a plain stream, a failed one and a missing device context with PGX_ESTATE.  pgx_dedup_close as above. */
int pgx_dedup_open_graph(uint64_t expected_pairs, pgx_dedup_stream **out);
int pgx_dedup_drain(pgx_dedup_stream *s, uint64_t max_lines, char **text, size_t *text_len, int *done);
int pgx_dedup_graph_stats(pgx_dedup_stream *s, uint64_t *n_contained_reads, uint64_t *n_lines_kept, uint64_t *n_lines_total);

/* ---- string graph (the first half of py/scripts/ovlp_to_graph.py: generate_string_graph, :658-905, with
 * disable_chimer_bridge_removal=True and lfc=False): from the rows a graph-mode dedup stream keeps in HBM to the sg_edges_list text,
 * byte-identical to the script's file.  Load filter (--min_len, --min_idt), edge construction (two edges per surviving row, numbered in
 * creation order: edge e's reverse is e ^ 1), transitive reduction, spur removal, best-overlap selection, spur removal again; the
 * file lists the edges in creation order, "%s %s %s %5d %5d %5d %5.2f %s\n" (:901).  All on the device, on the library's stream;
 * device memory is booked as "sgraph" (pgx_mem_ledger), time as "sgraph" (pgx_timing_get).
 *   pgx_sgraph_build : on a graph-mode stream after its last feed.  Runs the stream's final compaction if no drain has run yet (feeds are
 *                      refused afterwards, as after a drain); the rows stay with the stream, which can still be drained or closed, before
 *                      or after pgx_sgraph_free: the graph owns its arrays.  PGX_ESTATE: a plain or failed stream, or one whose last
 *                      line was drained (the rows are gone).  PGX_EINVAL, with a message that says why: any bit of `flags` but
 *                      PGX_SGRAPH_CHIMER_ORDERED (the chimer bridge step as the script runs it and --lfc are not offered: the first pops
 *                      from a set of objects, so the script's own output changes with the hash seed); more than 2^31 - 1 kept rows; a kept row with m_size == 0 (its identity prints as nan or
 *                      inf; the message names the row).  PGX_ENOMEM: no device memory -- the stream stays usable for pgx_dedup_drain.
 *                      A line whose first field is negative (a read id of 2^31 and more as rid0) would end the script's file; such rows
 *                      are built like any other here.
 *   pgx_sgraph_stats : the counts of the graph.
 *   pgx_sgraph_edges : n edge records from edge `first` on (first + n <= stats.edges), in creation order.
 *   pgx_sgraph_text  : the file in pieces with pgx_dedup_drain's conventions: the next lines, at most max_lines (> 0) and 2^24 per call,
 *                      *text malloc'd (pgx_free), *done != 0 with the last of them (at once for an empty graph).
 *   pgx_sgraph_free  : releases the graph (NULL is accepted).
 * PGX_SGRAPH_DEG_MAX (a test hook, read by every build): the most out-edges of a node whose transitive reduction runs from LDS tables
 * (default and maximum 256); nodes with more run the same pass on tables in HBM.
 *
 * PGX_SGRAPH_CHIMER_ORDERED: the script's chimer bridge step (mark_chimer_edges, :127-195 -- what the script does WITHOUT
 * --disable_chimer_bridge_removal, which is how pg_run.py runs it) between the transitive reduction and the first spur pass, with one
 * thing added to the script's algorithm: bfs_nodes (:107-125) pops from its pool the node with the smallest (rid as unsigned, end), B
 * before E, where the script pops from a set of objects.  The result is one of the script's own possible answers, and the script's
 * answer wherever the script has only one.  The rule: on the marks the reduction left, node n is a candidate iff some unreduced edge
 * u -> n has a tail with at least 2 unreduced out-edges and some unreduced edge n -> x a head with at least 2 unreduced in-edges.
 * With O the heads of all of n's out-edges and T the heads of all out-edges of the tails of n's in-edges, without n (edges in any
 * state), n is chosen iff O and T are disjoint and so are the unions of flow(v, n) over O and over T; flow(s, n): A = pool = {s}; at
 * most 4 times, while the pool is not empty, its smallest node p leaves it and every head w != n of p's out-edges that is not in A
 * enters A, and the pool too if w has out-edges.  Every edge of a chosen node that the reduction left unreduced is reduced with type
 * C, and so is its reverse; the later passes run on those marks.  A C edge prints `C`; pgx_sgraph_stats_t counts no C edges, so
 * n_g + n_tr + n_s + n_r falls short of `edges` by their number.  Accepted alone: with bit 1 or 2 those bits' refusals win.
 *   pgx_sgraph_chimer_stats : the step's counts; zeros for a graph built without the flag.
 *   pgx_sgraph_chimer_nodes : the chimers_nodes file (:854-856) as *text (pgx_free), *len bytes: for every chosen node, in node creation
 *                             order, its name and then its reverse end's, a line each.  The script's line order is that of a set of
 *                             objects: only the sorted lines compare.  Empty without the flag.
 * PGX_SGRAPH_CHIMER_LDS (a test hook, read by every build): the most nodes of a candidate's table in LDS (default and maximum 1024);
 * candidates whose flows reach more run the same tests on tables in HBM. */
#define PGX_SGRAPH_CHIMER_BRIDGE 1u   /* ask for the chimer bridge step as the script runs it (no single answer): refused */
#define PGX_SGRAPH_LFC 2u             /* ask for --lfc: refused */
#define PGX_SGRAPH_CHIMER_ORDERED 4u  /* the chimer bridge step with bfs_nodes' pool popped smallest (rid, end) first */
enum { PGX_SGRAPH_G = 0, PGX_SGRAPH_TR = 1, PGX_SGRAPH_S = 2, PGX_SGRAPH_R = 3, PGX_SGRAPH_C = 4 };
typedef struct {
  uint32_t v_rid, w_rid;     /* the edge leaves node (v_rid, v_end) and enters (w_rid, w_end) */
  uint32_t label_rid;
  int32_t sp, tp;            /* the label's coordinates; the edge's length is |sp - tp| */
  uint8_t v_end, w_end;      /* 0: B, 1: E */
  uint8_t type;              /* PGX_SGRAPH_G .. _C */
  uint8_t pad;
  int64_t score;             /* m_size */
  int64_t idt_tenths;        /* identity in tenths, as the dedup line prints it */
} pgx_sgraph_edge;
typedef struct {
  uint64_t rows_in, rows_pass;    /* kept rows of the stream; of them past --min_len / --min_idt */
  uint64_t edges, nodes;
  uint64_t n_g, n_tr, n_s, n_r;   /* edges by type */
  uint64_t max_out_degree;
  uint64_t spur_candidates;       /* nodes the spur pass visits */
} pgx_sgraph_stats_t;
typedef struct pgx_sgraph pgx_sgraph;
int pgx_sgraph_build(pgx_dedup_stream *s, int64_t min_len, double min_idt, uint32_t flags, pgx_sgraph **out);
int pgx_sgraph_stats(const pgx_sgraph *g, pgx_sgraph_stats_t *out);
int pgx_sgraph_edges(const pgx_sgraph *g, uint64_t first, uint64_t n, pgx_sgraph_edge *out);
int pgx_sgraph_text(pgx_sgraph *g, uint64_t max_lines, char **text, size_t *text_len, int *done);
int pgx_sgraph_free(pgx_sgraph *g);
typedef struct {
  uint64_t candidates;   /* nodes the step tests */
  uint64_t past_test1;   /* of them with O and T disjoint */
  uint64_t chosen;       /* of those with disjoint flows: the chimer nodes */
  uint64_t c_edges;      /* edges of type C */
} pgx_sgraph_chimer_stats_t;
int pgx_sgraph_chimer_stats(const pgx_sgraph *g, pgx_sgraph_chimer_stats_t *out);
int pgx_sgraph_chimer_nodes(const pgx_sgraph *g, char **text, size_t *len);

/* ---- unitigs (phase 1 of unitig construction in py/scripts/ovlp_to_graph.py: identify_simple_paths, :1033-1144): every maximal simple
 * path of the string graph's G edges as one unitig, and the `simple` lines of utg_data (:1478-1487).  Only edges of type G take part;
 * a node (rid, end) is simple when its G in-degree and out-degree are both 1.
 *   linear    every G edge that leaves a non-simple node starts a unitig; it follows the single out-edge of each simple node it reaches
 *             and ends at the first non-simple node (which may be the start node: s == t, not circular).
 *   circular  what no such start reaches lies on rings of simple nodes: a ring is one unitig, cut at the tail of its edge with the
 *             smallest creation index; its path is closed (the first node again at the end).
 *   fields    length = the sum of |sp - tp|, score = the sum of the edges' scores; via = the path's SECOND node (the script's via is the
 *             second or the second-to-last node, whichever of a path and its reverse it happens to walk: it varies with the hash seed,
 *             as do the order of the unitigs and the place where a ring is opened).
 *   order     every directed G edge lies in exactly one unitig (a path and its reverse are two); unitigs are numbered, and lines written,
 *             in ascending creation index of their first edge.
 *   line      "s via t simple length score n0~n1~...~nk\n", node names as in sg_edges_list ("%09d" of the signed rid, ":B" or ":E").
 * The later phases of the script (unitig spurs, duplicate paths, compound paths, contig paths) pop from sets of strings: they are offered
 * with every such container given an order, below ("contig paths").
 * All on the device, on the library's stream: one sort per edge list, list ranking by pointer doubling (a logarithmic number of passes
 * whatever the length of a path), no launch per unitig.  Device memory is booked as "unitigs", time as "unitigs" with the parts
 * "unitigs_links", "unitigs_rank", "unitigs_paths", "unitigs_text".
 *   pgx_sgraph_unitigs : of a built graph, whose edges stay on the device.  The unitigs own their arrays: the graph may be freed first.
 *   pgx_unitigs_build  : of n host edge records in creation order (a parsed sg_edges_list, whoever wrote it); `type` != PGX_SGRAPH_G
 *                        is ignored.  Fewer than 2^31 records.
 *     Both check what the script asserts, and answer PGX_EINVAL with a message that names the smallest offending edge index: a G edge
 *     with v_rid == w_rid; a G edge whose (v, w) an earlier G edge has; a G edge (v, w) without its reverse (rev w, rev v) among the
 *     G edges.  PGX_ENOMEM: no device memory (the graph stays usable).  No G edge: zero unitigs, an empty text.
 *   pgx_unitigs_stats  : the counts.            pgx_unitigs_table : n table entries from unitig `first` on.
 *   pgx_unitigs_paths  : n entries of the path array from entry `first` on (g_edges in all): creation indices of the edges, unitig after
 *                        unitig; unitig u's are [table[u].first, + table[u].n_edges).
 *   pgx_unitigs_text   : the lines in pieces, with pgx_sgraph_text's conventions (at most max_lines (> 0) and 2^24 lines per call).
 *   pgx_unitigs_free   : releases them (NULL is accepted).
 * After pgx_shutdown every call but pgx_unitigs_free answers PGX_ESTATE, as for graphs. */
typedef struct {
  uint32_t s_rid, t_rid, via_rid;              /* first, last and second node of the path */
  uint8_t s_end, t_end, via_end, circular;     /* 0: B, 1: E; circular: a ring of simple nodes */
  uint32_t n_edges;
  uint64_t first;                              /* offset of its first edge in the path array */
  int64_t length, score;
} pgx_unitig;
typedef struct {
  uint64_t g_edges, unitigs, circular, longest_edges;
} pgx_unitigs_stats_t;
typedef struct pgx_unitigs pgx_unitigs;
int pgx_sgraph_unitigs(pgx_sgraph *g, pgx_unitigs **out);
int pgx_unitigs_build(const pgx_sgraph_edge *edges, uint64_t n, pgx_unitigs **out);
int pgx_unitigs_stats(const pgx_unitigs *u, pgx_unitigs_stats_t *out);
int pgx_unitigs_table(const pgx_unitigs *u, uint64_t first, uint64_t n, pgx_unitig *out);
int pgx_unitigs_paths(const pgx_unitigs *u, uint64_t first, uint64_t n, uint32_t *edge_index);
int pgx_unitigs_text(pgx_unitigs *u, uint64_t max_lines, char **text, size_t *text_len, int *done);
int pgx_unitigs_free(pgx_unitigs *u);

/* ---- reads -> contigs mapping (replaces shmr_map, src/shmr_map.c:48-161,163-373) ----
 * The reads' shimmer-pair map is built exactly as in the overlap stage (build_map with -t/-c/-n/-M); the reference
 * shimmers are chained the same way and every hit bucket is reported, one line per record in insertion order:
 * "ref_id ref_bgn ref_end read_id read_bgn read_end direction mcount0 mcount1\n" (shmr_map.c:152-153).  *text is malloc'd
 * (pgx_free) and byte-identical to the reference's stdout. */
typedef struct {
  int total_chunk, mychunk;  /* -t -c */
  int mc_lower, mc_upper;    /* -n -M (defaults 1, 240: shmr_map.c:28-29) */
} pgx_map_params;
int pgx_map(const pgx_mm128 *ref_mmers, size_t n_ref, const pgx_mm128 *mmers, size_t n_mm, const pgx_mm_count *counts,
            size_t n_counts, const uint32_t *rlen_by_rid, uint32_t n_rid, const pgx_map_params *p, char **text,
            size_t *text_len, uint64_t *n_lines);
/* file level: -r refdb_prefix (unused, as in the reference) -m ref_shimmer_prefix -p seqdb_prefix -l shimmer_prefix */
int pgx_map_chunk(const char *refdb_prefix, const char *ref_shimmer_prefix, const char *seqdb_prefix,
                  const char *shimmer_prefix, const pgx_map_params *p, char **text, size_t *text_len, uint64_t *n_lines);
/* pgx_map / pgx_map_chunk answering the rows in place of the text: *rows (pgx_free) holds *n_rows x 9 int64, a line's nine numbers in the
 * order the text has them -- what pgx_map_merge_rows and pgx_cns_job_resident take, so a resident caller never forms the text. */
int pgx_map_rows(const pgx_mm128 *ref_mmers, size_t n_ref, const pgx_mm128 *mmers, size_t n_mm, const pgx_mm_count *counts,
                 size_t n_counts, const uint32_t *rlen_by_rid, uint32_t n_rid, const pgx_map_params *p, int64_t **rows,
                 uint64_t *n_rows);
int pgx_map_rows_chunk(const char *refdb_prefix, const char *ref_shimmer_prefix, const char *seqdb_prefix,
                       const char *shimmer_prefix, const pgx_map_params *p, int64_t **rows, uint64_t *n_rows);

/* ---- map merge (replaces `cat map-*.dat | sort -k 1 -g -k 2 -g`, pg_run.py:491-496, the step between shmr_map and pg_asm_cns.py) ----
 * The order is that of `LC_ALL=C sort -k 1 -g -k 2 -g` on shmr_map's lines (nine canonical decimals below 2^32, single blanks): by field
 * 0 as a number, by field 1 as a number, then by the whole line bytewise -- fields 2 .. 8 compared as decimal STRINGS ("100" before
 * "99", "7" before "70").  Rows equal under all three are identical lines.  One stable 64-bit radix sort by (field 0, field 1), then the
 * runs of equal keys by the string rule: a run of up to 64 rows on a wavefront, one of up to 1,024 on a workgroup, longer ones through
 * an LSD sort of their rows alone.  n < 2^31 rows; no host spill: rows that do not fit the device answer
 * PGX_ENOMEM.  PGX_MERGE_RUN_MAX=<rows> (1 .. 1,024) shrinks the workgroup's bound -- below 64 the wavefront's too; 1 sends every tie run
 * through the LSD sort -- and PGX_MERGE_PIECE=<bytes> the pieces of the file level: test hooks. */
typedef struct {
  uint64_t n_rows, n_runs, n_tie_runs, longest_run;   /* runs of equal (field 0, field 1); those of two rows and more; the longest */
  uint64_t rows_wave, rows_group, rows_lsd;           /* rows of tie runs by the path that ordered them */
  double parse_ms, key_ms, sort_ms, ties_ms, format_ms;   /* host clock: text to rows, keys, the radix sort, the runs + gather, rows to text */
} pgx_map_merge_stats;                                /* 96 bytes */
/* rows: n x 9 uint32 in device memory, any order; the merged rows to d_out (device, n x 9, not d_rows) */
int pgx_map_merge_dev(const uint32_t *d_rows, uint64_t n, uint32_t *d_out, pgx_map_merge_stats *stats);
/* the host form, n x 9 int64 in, n x 9 int64 out (the caller's array; may be `rows`).  A value outside [0, 2^32): PGX_EINVAL, the row named. */
int pgx_map_merge_rows(const int64_t *rows, size_t n, int64_t *out, pgx_map_merge_stats *stats);
/* the file level: the map chunk files, one after the other in the given order ("-": stdin), to one merged file (out_path NULL: stdout).
 * Parsed on the device in bounded pieces of each file, the rows kept there as 9 x u32, the text formatted there in bounded pieces.
 * PGX_EINVAL, the file and the 0-based line named and NOTHING written: a line that is not nine canonical decimals (0|[1-9][0-9]*) below
 * 2^32 separated by single blanks -- a sign, a leading zero, a tab, a '\r', a blank line, eight or ten fields.  A file's last line may
 * lack its '\n' (the output ends every line with one); empty files and no rows at all give an empty output. */
int pgx_map_merge(const char *const *paths, size_t n_paths, const char *out_path, pgx_map_merge_stats *stats);

/* ---- batch level ---- */
/* pgx_sketch_batch with mm_sketch's is_hpc = 1 (any 0 < k <= 28, 0 < w < 256): same arguments, same ownership */
int pgx_sketch_batch_hpc(pgx_seqdb *db, const uint32_t *read_slots, uint32_t n, int w, int k, pgx_mm128 **out, size_t *n_out);
int pgx_sketch_batch(pgx_seqdb *db, const uint32_t *read_slots, uint32_t n, int w, int k, pgx_mm128 **out,
                     size_t *n_out);  /* read_slots index the idx-file order; output in that order */
int pgx_reduce_batch(const pgx_mm128 *in, size_t n, int rs, pgx_mm128 **out, size_t *n_out);
int pgx_count_batch(const pgx_mm128 *in, size_t n, pgx_mm_count **out, size_t *n_out);
int pgx_align_batch(pgx_seqdb *db, const pgx_align_key *keys, size_t n, int band, pgx_match *out);
/* pgx_align_key plus an offset into the TARGET: target = read rid1 from byte t_off to its end (the arguments path_to_contig.py passes to
 * ovlp_match, py/scripts/path_to_contig.py:80-84).  Runs nibble by nibble on the reads' bytes in every state of the database: after
 * pgx_seqdb_release_bytes / _compact_bytes on a byte view of the reads the keys name, rebuilt from the packs for the call. */
typedef struct { uint32_t rid0, rid1, q_off, t_off; uint8_t dir0, dir1, pad[2]; } pgx_align_key2; /* 20 bytes */
int pgx_align_batch2(pgx_seqdb *db, const pgx_align_key2 *keys, size_t n, int band, pgx_match *out);

/* ---- contig layout (replaces py/scripts/path_to_contig.py, run twice by py/scripts/pg_run.py:356-362) ----
 * One row of a tiling path: `ctg_id v w r s e olen idt _ _` with v = rid0:E|B, w = rid1:E|B (strand 0 for E, 1 otherwise) and s, e as the
 * file gives them.  ctg numbers the contigs 0 .. n_ctg - 1 in order of first appearance; the rows of a contig are consecutive, in file
 * order.  Per contig the first row's read v is laid down whole at 0; every row (the first included) aligns the last 500 bases of v to the
 * last |e - s| + 500 of w (band 100) and appends seg = e - s + 500 - t_m_end bytes of w that end at e (s, e = rlen - s, rlen - e on
 * strand 1) at ctg_len - 500 + q_m_end; later rows overwrite earlier ones, bytes no segment covers are 'N'.
 *   pgx_contigs_resident : the contig bytes only, contig c at (*text)[ctg_off[c] .. ctg_off[c + 1]) (ctg_off: n_ctg + 1 entries, caller's);
 *                          *text is malloc'd (pgx_free).  Any state of the database (bytes / released / compacted).
 *   pgx_contigs_chunk    : the file level -- <seqdb_prefix>.idx / .seqdb and the tiling path in, FASTA (">ctg_id\n" contig "\n") to out_path
 *                          (NULL: stdout), byte for byte the script's stdout.  Only the reads the path names are uploaded, in batches of
 *                          whole contigs that fit HBM (PGX_CONTIGS_BATCH=<contigs per batch>: a test hook).
 * PGX_EARG, a message that names the row (0-based, in file order), nothing written -- where the script raises or reads out of bounds: a
 * row without 10 fields or with an unparsable s / e, a rid the idx lacks, len(v) < 500, |e - s| + 500 > len(w), e <= s after the strand
 * transform, and -- known after the alignment, the first such row is reported -- e - seg < 0, a segment that starts before 0 or ends
 * beyond the end of its contig. */
typedef struct { uint32_t ctg, rid0, rid1; int32_t s, e; uint8_t strand0, strand1, pad[2]; } pgx_tile_row; /* 24 bytes */
int pgx_contigs_resident(pgx_seqdb *db, const pgx_tile_row *rows, size_t n_rows, size_t n_ctg, char **text, uint64_t *ctg_off,
                         uint64_t *text_len);
int pgx_contigs_chunk(const char *seqdb_prefix, const char *tiling_path, const char *out_path, uint64_t *n_ctg, uint64_t *n_bases);

/* ---- contig paths (the phases of py/scripts/ovlp_to_graph.py after identify_simple_paths, :1147-1555): from the unitigs to the final
 * utg_data (:1478-1487) and ctg_paths (:1496-1555).  The script pops from sets of strings, so its files vary with PYTHONHASHSEED; the
 * rule here is the script's algorithm with every unordered container given an order -- a node is its key
 * (rid << 1) | end, a unitig its index (pgx_unitigs' numbering; compound unitigs follow in order of creation), sets pop their smallest
 * element, a node's edges iterate in ascending unitig index -- and equals the script wherever the script has one answer, with one
 * exception: where the script removes a spur it writes the spur's own length, score and path over its dual's entry (:1210-1212); here the
 * dual's `spur:2` line keeps its own.  `via` stays
 * the path's second node; a unitig's reverse is its DUAL by structure (the unitig that starts with the reverse of its last edge; a ring
 * has none: PGX_CTG_NONE).  Chimer bridge removal and --lfc are off; c_path, chimers_nodes and utg_data0 are not written.
 *   pgx_unitigs_contig_paths : of live unitigs (either builder's).  The unitigs are not changed; the simple lines of utg_data read their
 *                              path arrays, so pgx_ctg_paths_utg_text answers PGX_ESTATE once they are freed (the rest keeps working).
 *   pgx_ctg_paths_build      : of n host edge records in creation order (a parsed sg_edges_list, whoever wrote it): pgx_unitigs_build
 *                              (its checks, its messages), then the above; the unitigs belong to the result.
 *     PGX_EINVAL where the script asserts or raises, with the unitig or node named: a unitig without a dual, two short s == t loops at one
 *     node, a bundle in which no in-edge has a positive score, a repeat bridge whose dual left the graph.  PGX_ENOMEM: no device memory
 *     (the unitigs stay as they were).
 *   pgx_ctg_paths_stats  : the counts; spur_rounds: paths removed by the two spur passes; host_us: the serial cascades over the unitig
 *                          table, which run on the host; device_walks: contig walks made on the device (a lane per start edge):
 *                          all that leave a start node, unless walks sharing a stretch are still unsettled after 64 rounds -- those go to the host,
 *                          and which ones they are may differ from run to run (the files never do).
 *   pgx_ctg_paths_table  : n entries from unitig `first` on (stats.unitigs in all): final type (PGX_CTG_*) and dual.
 *   pgx_ctg_paths_rows   : the unitig lists of the lines of ctg_paths, as indices: line l's are unitig[row_off[l] .. row_off[l + 1])
 *                          (row_off: ctg_lines + 1 entries, unitig: row_entries; either may be NULL).
 *   pgx_ctg_paths_utg_text / _ctg_text : the lines of the two files in pieces, with pgx_sgraph_text's conventions; each keeps its own place.
 *   pgx_ctg_paths_free   : releases them (NULL is accepted).
 * After pgx_shutdown every call but pgx_ctg_paths_free answers PGX_ESTATE.  Device memory is booked as "ctg_paths", time as "ctg_paths"
 * with the parts "ctg_paths_graph", "ctg_paths_clean", "ctg_paths_walk", "ctg_paths_text". */
enum { PGX_CTG_SIMPLE = 0, PGX_CTG_SPUR2 = 1, PGX_CTG_SIMPLE_DUP = 2, PGX_CTG_CONTAINED = 3, PGX_CTG_REPEAT_BRIDGE = 4, PGX_CTG_COMPOUND = 5 };
#define PGX_CTG_NONE 0xFFFFFFFFu
typedef struct {
  uint32_t type, dual;
} pgx_ctg_unitig;
typedef struct {
  uint64_t unitigs, simple, spur2, simple_dup, contained, repeat_bridge, compound, ctg_linear, ctg_circular, ctg_lines, row_entries, longest_ctg, spur_rounds, host_us, device_walks;
} pgx_ctg_paths_stats_t;
typedef struct pgx_ctg_paths pgx_ctg_paths;
int pgx_unitigs_contig_paths(pgx_unitigs *u, pgx_ctg_paths **out);
int pgx_ctg_paths_build(const pgx_sgraph_edge *edges, uint64_t n, pgx_ctg_paths **out);
int pgx_ctg_paths_stats(const pgx_ctg_paths *c, pgx_ctg_paths_stats_t *out);
int pgx_ctg_paths_table(const pgx_ctg_paths *c, uint64_t first, uint64_t n, pgx_ctg_unitig *out);
int pgx_ctg_paths_rows(const pgx_ctg_paths *c, uint64_t *row_off, uint32_t *unitig);
int pgx_ctg_paths_utg_text(pgx_ctg_paths *c, uint64_t max_lines, char **text, size_t *text_len, int *done);
int pgx_ctg_paths_ctg_text(pgx_ctg_paths *c, uint64_t max_lines, char **text, size_t *text_len, int *done);
int pgx_ctg_paths_free(pgx_ctg_paths *c);

/* ---- tiling paths (replaces py/scripts/graph_to_path.py, pg_run.py:355): from sg_edges_list, utg_data and ctg_paths to p_ctg_tiling_path
 * and a_ctg_tiling_path, byte for byte the script's files, and to the same rows as pgx_tile_row ("tiling paths", states the rule).
 *   pgx_sgraph_parse : a sg_edges_list file as edge records in the file's order, tokenised on the device (the file goes up in pieces of
 *                      PGX_TILING_PIECE bytes, default and maximum 1 GiB, a test hook; a lane per line).  Blank lines are skipped; types
 *                      other than G, TR, S, R become 4.  *edges and *idt_hundredths (may be NULL) are the caller's (pgx_free);
 *                      idt_tenths is the identity's exact decimal rounded half to even.
 *   pgx_tiling_build : sg_edges_list_fn, or a built graph g whose edges stay on the device (exactly one of the two), plus the texts of
 *                      utg_data and ctg_paths.  The tiling paths own their arrays: the graph may be freed first.
 *   pgx_tiling_stats : the counts.  ctg_kept + ctg_skipped + ctg_empty = the rows of ctg_paths; compound_tie_rounds: the shortest-path
 *                      rounds in which more than one path had the minimum weight (0: the output is the script's under any networkx;
 *                      else ours is forward Dijkstra's); host_us: the host's time over utg_data, ctg_paths and the bundles.
 *   pgx_tiling_rows  : n rows of file `which` (0: primary, 1: alternate) from row `first` on; `ctg` numbers the distinct contig names of
 *                      that file in order of first appearance, strand 0 for E, 1 for B.
 *   pgx_tiling_names : those names, a line each (*text malloc'd, pgx_free).
 *   pgx_tiling_text  : the lines of file `which` in pieces, with pgx_sgraph_text's conventions.
 *   pgx_tiling_contigs : contig FASTA of file `which` from the rows of the built tiling and <seqdb_prefix>.idx / .seqdb, to out_path (NULL:
 *                      stdout): byte for byte pgx_contigs_chunk's on the written file, with its errors (rows are numbered as its lines).  The
 *                      24-byte rows come to the host once; no text is written and parsed again.
 *   pgx_tiling_free  : releases them (NULL is accepted).
 *   pgx_tiling_chunk : the file level; both files are written only after everything was built.
 * PGX_EINVAL with a message that names the file and the 0-based line, and nothing written, where the script would raise: a line of
 * sg_edges_list without 8 fields or of the other two without 7; a G line whose w does not end in E for s < t, in B otherwise; a unitig
 * that a kept row of ctg_paths or a compound line names and utg_data lacks as simple, contained or compound; an edge of a path that is
 * not a G line; a compound sub-unitig that is itself compound; s or t absent from a compound unitig's graph, or no path between them.
 * Beyond the script: a field that would not print back as it was read (a node name that is not "%09d:B|E" of a read id below 2^31, an
 * identity with more than two fraction digits, an exponent, nan; in G lines only, the script reads no more of the others -- pgx_sgraph_parse
 * checks every line); a line of sg_edges_list longer than 256 bytes; a (v, w) or (s, via, t) that occurs twice (the later line is named:
 * the script's dicts would keep it, its own files never repeat a key); a compound unitig's edge with aln_score <= 0 or >= 2^40, or one with s == t; a
 * path of one node (the script writes an empty line); a contig name longer than 89 bytes.  PGX_ENOMEM leaves the inputs usable.
 * Device memory is booked as "tiling", time as "tiling" with the parts "tiling_parse", "tiling_index", "tiling_paths", "tiling_text". */
typedef struct {
  uint64_t sg_lines, g_edges;                       /* edge lines read; of them G */
  uint64_t utg_simple, utg_contained, utg_compound; /* lines of utg_data by type (other types are dropped) */
  uint64_t ctg_kept, ctg_skipped, ctg_empty;        /* rows of ctg_paths: written; dropped by the dual rule; kept with an empty path */
  uint64_t p_rows, a_rows, alternates;              /* lines of the two files; paths of the alternate file */
  uint64_t compound_tie_rounds;
  uint64_t host_us;
} pgx_tiling_stats_t;
typedef struct pgx_tiling pgx_tiling;
int pgx_sgraph_parse(const char *sg_edges_list_fn, pgx_sgraph_edge **edges, int64_t **idt_hundredths, uint64_t *n);
int pgx_tiling_build(const char *sg_edges_list_fn, pgx_sgraph *g, const char *utg_text, size_t utg_len, const char *ctg_text, size_t ctg_len, pgx_tiling **out);
int pgx_tiling_stats(const pgx_tiling *t, pgx_tiling_stats_t *out);
int pgx_tiling_rows(const pgx_tiling *t, int which, uint64_t first, uint64_t n, pgx_tile_row *out);
int pgx_tiling_names(const pgx_tiling *t, int which, char **text, size_t *text_len, uint64_t *n_ctg);
int pgx_tiling_text(pgx_tiling *t, int which, uint64_t max_lines, char **text, size_t *text_len, int *done);
int pgx_tiling_contigs(const pgx_tiling *t, int which, const char *seqdb_prefix, const char *out_path, uint64_t *n_ctg, uint64_t *n_bases);
int pgx_tiling_free(pgx_tiling *t);
int pgx_tiling_chunk(const char *sg_edges_list_fn, const char *utg_data_fn, const char *ctg_paths_fn, const char *p_out, const char *a_out, pgx_tiling_stats_t *stats);

/* ---- assembly graph as GFA 1.0 (no counterpart in the reference workflow): the phase-1 unitigs (above: every directed G
 * edge lies in exactly one unitig, a path and its reverse are two) as segments with sequences, and the links between them.  The rule:
 *   dual      dual(u) is the unitig that holds the reverse of u's first edge: edge e ^ 1 in a built graph, the edge (rev w, rev v) among
 *             host records.  dual(dual(u)) == u and dual(u) != u follow from what pgx_unitigs checks; violations are counted on the device
 *             and any is PGX_ESTATE: no wrong file is written.
 *   segments  u is canonical iff u < dual(u); every canonical unitig is one segment, numbered densely in ascending unitig index and named
 *             "utg%06u" of the unitig's index -- the 0-based number of its line in pgx_unitigs_text.  A directed unitig x prints as the name
 *             of min(x, dual(x)) and '+' if x is canonical, else '-'.
 *   rows      segment j of canonical unitig u has one pgx_tile_row per edge of u's path, in path order (a ring's closing edge included: the
 *             first read's bases come again at the end): ctg = j, rid0 = v_rid, rid1 = w_rid, s = sp, e = tp, strand0 = 1 - v_end,
 *             strand1 = 1 - w_end.
 *   sequences (only with a database) a segment's bases are what the contig layout (above, "contig layout") makes of its rows; a row the
 *             layout refuses is PGX_EARG, the message names the segment, the position in its path and the edge index.
 *   links     for every ordered pair of directed unitigs (a, b) with t(a) == s(b), a == b included, there is a directed link; a's links
 *             are the G out-edges of node t(a), each the first edge of a unitig.  The dual of (a, b) is (dual b, dual a), never the same
 *             pair; of the two the lexicographically smaller pair of unitig indices is written.  Links ascend by (a, b).
 *   text      "H\tVN:Z:1.0\n"; per segment "S\t<name>\t<bases>\tLN:i:<number of bases>\n", or "S\t<name>\t*\n" without a database (no
 *             length is invented: a unitig's `length` excludes its first read); per link "L\t<name a>\t<+|->\t<name b>\t<+|->\t*\n" -- the
 *             overlap is '*' on purpose: the end of a and the start of b come from one read through different stitching alignments.
 *             No G edge: the header line alone.
 *   pgx_gfa_build : u, and the edge records u was built from: a live graph g, or n_edges host records in creation order -- exactly one of
 *                   the two (else PGX_EARG); db: a resident read database in any state (bytes, released, compacted), or NULL for the
 *                   topology-only file.  PGX_EARG: the records' G count differs from u's g_edges, a path index lies beyond the records,
 *                   a path's edge is not the G edge the unitigs saw there.  PGX_ENOMEM: the inputs stay usable.  The result owns its
 *                   arrays: u, g and db may be freed first.
 *   pgx_gfa_build_files : the file level -- the same with the sequences from <seqdb_prefix>.idx / .seqdb (NULL: the topology-only file):
 *                   only the reads the rows name are uploaded, in pgx_contigs_chunk's batches of whole segments that fit HBM.
 *   pgx_gfa_stats / _segments / _links / _rows : the counts, and n table entries from entry `first` on.
 *   pgx_gfa_text  : the whole file, malloc'd (pgx_free).      pgx_gfa_write : to a file (NULL: stdout).
 *   pgx_gfa_free  : releases it (NULL is accepted).
 * After pgx_shutdown every call but pgx_gfa_free answers PGX_ESTATE.  Device memory is booked as "gfa", time as "gfa" with the parts
 * "gfa_dual", "gfa_rows", "gfa_links", "gfa_text" (the layout's parts keep their names). */
typedef struct { uint32_t unitig, dual; uint32_t n_rows; uint8_t circular, pad[3]; uint64_t first_row, seq_off, seq_len; } pgx_gfa_segment; /* 40 bytes */
typedef struct { uint32_t from_seg, to_seg; uint8_t from_rev, to_rev, pad[2]; } pgx_gfa_link;                                         /* 12 bytes */
typedef struct { uint64_t unitigs, segments, rows, links_directed, links, bases; } pgx_gfa_stats_t;
typedef struct pgx_gfa pgx_gfa;
int pgx_gfa_build(pgx_unitigs *u, pgx_sgraph *g, const pgx_sgraph_edge *edges, uint64_t n_edges, pgx_seqdb *db, pgx_gfa **out);
int pgx_gfa_build_files(pgx_unitigs *u, pgx_sgraph *g, const pgx_sgraph_edge *edges, uint64_t n_edges, const char *seqdb_prefix, pgx_gfa **out);
int pgx_gfa_stats(const pgx_gfa *f, pgx_gfa_stats_t *out);
int pgx_gfa_segments(const pgx_gfa *f, uint64_t first, uint64_t n, pgx_gfa_segment *out);
int pgx_gfa_links(const pgx_gfa *f, uint64_t first, uint64_t n, pgx_gfa_link *out);
int pgx_gfa_rows(const pgx_gfa *f, uint64_t first, uint64_t n, pgx_tile_row *out);
int pgx_gfa_text(pgx_gfa *f, char **text, size_t *len);
int pgx_gfa_write(pgx_gfa *f, const char *path);
int pgx_gfa_free(pgx_gfa *f);

/* ---- consensus call: the second half of pg_asm_cns.py's inner loop (py/scripts/pg_asm_cns.py:149-242), get_align_tags and
 * get_cns_from_align_tags of falcon/falcon.c:67-122,277-397, for a batch of pieces at once.  An alignment is what falcon.align answers for
 * one read against a piece: the two alignment strings (str_len bytes each at str_off of q_str and of t_str, over ACGTNacgtn and '-'), its
 * start pair and the offset of the aligned template part in the piece.  The consensus of a piece is a function of the multiset of its
 * alignments: rows may come in any order.  Where the reference has no answer the call refuses with PGX_EINVAL and names the piece: no
 * alignment path scoring above zero (the reference reads through an end iterator), a tag at or past the template's end, a negative
 * t_offset, more than 65,535 alignments in a piece (its counters are 16-bit), a byte outside ACGTNacgtn- in an alignment string. ---- */
typedef struct { uint32_t piece; int32_t t_offset, s1, s2; uint64_t str_off; uint32_t str_len, pad; } pgx_cns_aln;   /* 32 bytes */
/* one column of an alignment as the reference tags it (align_tag_t): its own position and the previous column's */
typedef struct { int32_t t_pos, p_t_pos; uint8_t delta, q_base, p_delta, p_q_base; } pgx_cns_tag;                  /* 12 bytes */
typedef struct {
  uint64_t n_aln, n_tags, n_edges, n_nodes, text_bytes;
  double gpu_ms, tags_ms, sort_ms, score_ms, back_ms;   /* the whole call on the device; its tag, sort, scoring and back-track parts */
} pgx_cns_stats;
/* *text (pgx_free): the pieces' consensus sequences back to back, piece p at [piece_off[p], piece_off[p + 1]) (n_piece + 1 entries);
 * lower case where the coverage is at most min_cov.  All arrays are the host's. */
int pgx_cns_call(const pgx_cns_aln *alns, size_t n_aln, const char *q_str, const char *t_str, size_t str_bytes, const uint32_t *piece_tlen,
                 size_t n_piece, uint32_t min_cov, char **text, uint64_t *piece_off, pgx_cns_stats *stats);
/* the same with the rows and both strings in device memory (what an aligner on the device leaves); piece_tlen and the results are the host's */
int pgx_cns_call_dev(const pgx_cns_aln *d_alns, size_t n_aln, const char *d_q_str, const char *d_t_str, size_t str_bytes, const uint32_t *piece_tlen,
                     size_t n_piece, uint32_t min_cov, char **text, uint64_t *piece_off, pgx_cns_stats *stats);
/* the tags alone: *tags (pgx_free) holds alignment a's at [tag_off[a], tag_off[a + 1]) (n_aln + 1 entries); `piece` is not read */
int pgx_cns_tags(const pgx_cns_aln *alns, size_t n_aln, const char *q_str, const char *t_str, size_t str_bytes, pgx_cns_tag **tags, uint64_t *tag_off);

/* ---- falcon.align: the first half of that loop, the banded O(ND) aligner with trace-back of falcon/DW_banded.c:104-315, for a batch of
 * requests over one pool of bytes.  Bytes are compared as bytes ('a' != 'A', 'N' == 'N').  A request that does not align -- the band grew
 * wider than 2 * band, or 0.3 * (q_len + t_len) steps did not reach an end of either sequence -- answers all zero, as the reference does.
 * band <= 4096 (the front keeps 2 * band + 4 diagonals, rounded up to a power of two, in LDS: at most 16,384 slots, 64 KiB).
 * The script itself -- contig chunking, read grouping, the stitching of the pieces -- is pgx_cns_job, further down. ---- */
typedef struct { uint64_t q_off, t_off; uint32_t q_len, t_len, band, want_str; } pgx_faln_req;                       /* 32 bytes */
typedef struct { int32_t aln_str_size, dist, aln_q_s, aln_q_e, aln_t_s, aln_t_e; uint64_t str_off; } pgx_faln_res;  /* 32 bytes */
typedef struct {
  uint64_t n_req, n_aligned, n_cells, str_bytes;   /* requests, those that reached an end, trace cells kept (4 bytes each), bytes per string buffer */
  double gpu_ms, count_ms, fill_ms, back_ms;       /* the aligner on the device; its counting pass, filling pass and trace-back */
} pgx_faln_stats;
/* falcon.align for n requests over one pool of bytes (host arrays).  *q_str, *t_str (pgx_free): request r's strings at
 * [str_off, str_off + aln_str_size) of both where want_str != 0 and it aligned; otherwise it owns no bytes. */
int pgx_falcon_align(const pgx_faln_req *reqs, size_t n, const char *seq, size_t seq_bytes, pgx_faln_res *res,
                     char **q_str, char **t_str, uint64_t *str_bytes, pgx_faln_stats *stats);

typedef struct { uint64_t seq_off; uint32_t t_len, pad; } pgx_cns_piece;                                      /* 16 bytes */
typedef struct { uint64_t seq_off; uint32_t seq_len, piece; int32_t read_shift; uint32_t pad; } pgx_cns_read; /* 24 bytes */
typedef struct {
  pgx_faln_stats align;                            /* the back-bones' and the reads' alignments */
  uint64_t n_pieces, n_reads, n_accepted, n_rejected, n_by_rule, n_called;   /* reads by the acceptance rule; pieces answered by the
                                                                                 low-coverage rule and by the consensus call */
  pgx_cns_stats call;
} pgx_cns_pieces_stats;
/* pg_asm_cns.py:143-244 for a batch of pieces: text / piece_off as pgx_cns_call; read_used[r] (may be NULL) = 1 where read r was accepted.
 * Per piece the back-bone (the template against itself, band 50), then every read at band 150: a read with read_shift < 0 without its
 * first -read_shift bases against the template, one with read_shift >= 0 against the template from read_shift on; accepted where the
 * aligned query span comes within 48 of the query (or, read_shift >= 0, of what is left of the template).  A piece whose accepted reads
 * cover fewer than 3 * t_len template bases answers its template in lower case; the others go through the consensus call, whose
 * refusals pass through (PGX_EINVAL, the piece named).  A read clipped to nothing is skipped.  PGX_EINVAL also for t_len == 0. */
int pgx_cns_pieces(const pgx_cns_piece *pieces, size_t n_piece, const pgx_cns_read *reads, size_t n_read, const char *seq, size_t seq_bytes,
                   uint32_t min_cov, char **text, uint64_t *piece_off, uint8_t *read_used, pgx_cns_pieces_stats *stats);

/* ---- pg_asm_cns.py as a whole (py/scripts/pg_asm_cns.py; the rule: DESIGN.md section 4.7b).  A map row is nine integers
 * `ctg p1 p2 read rb re strand mc0 mc1` (int64 each).  The layout: a contig's rows, sorted stably by p1, are cut into groups -- a row
 * 50,000 and more beyond the group's left anchor closes it and is the next anchor; a group that grew to 100,000 and more is emptied; a
 * tail of at most 1,000 goes to the group before -- and every group is a piece whose template is the contig's bases
 * [left, left + t_len) = [left_anchor - 1000, right).  Its read entries: per (read, strand) an entry at the smallest offset p1 - rb and at
 * every offset more than 50 above the last entry's, read_shift = offset - left, in the order the script aligns them.  Pieces come contig by
 * contig in the order of first appearance among the rows, a contig's segments in order; piece p owns reads [read_first, read_first + n_read).
 * Refused with PGX_EINVAL, the row or the contig and segment named: a contig the lengths lack (ctg_len[ctg] < 0 or ctg >= n_ctg) or of
 * length 0, a template that is empty or leaves its contig, and what the tables cannot hold (|p1| or |rb| or a length of 2^29 and more, a
 * read id beyond 32 bits, a strand other than 0 and 1). ---- */
typedef struct { uint32_t ctg, seg; int32_t left; uint32_t t_len, n_mapped, read_first, n_read, pad; } pgx_cns_job_piece;   /* 32 bytes */
typedef struct { uint32_t piece, read; int32_t read_shift; uint32_t strand; } pgx_cns_job_read;                             /* 16 bytes */
/* the layout alone: rows (n_rows x 9, the chunk's) and the contig lengths by contig id in, *pieces and *reads (pgx_free) out */
int pgx_cns_layout(const int64_t *rows, size_t n_rows, const int64_t *ctg_len, size_t n_ctg, pgx_cns_job_piece **pieces, uint64_t *n_piece,
                   pgx_cns_job_read **reads, uint64_t *n_read);
typedef struct {
  uint64_t n_rows, n_contigs, n_pieces, n_reads;     /* rows kept by the chunk filter, contigs answered, pieces, read entries */
  uint64_t n_accepted, n_by_rule, n_called;          /* entries the acceptance rule kept; pieces by the low-coverage rule / the call */
  uint64_t n_batches, pool_bytes, text_bytes;        /* batches of pieces, ASCII pool bytes decoded over all of them, FASTA bytes */
  double total_ms, layout_ms, decode_ms, pieces_ms, stitch_ms;   /* host clock around the parts: layout, decode, inner loop, stitch + FASTA */
  pgx_faln_stats align;                              /* the aligner's, summed over the batches and the stitch */
  pgx_cns_stats call;                                /* the call's, summed over the batches */
} pgx_cns_job_stats;
/* The script on two resident databases (their bytes in place: not released, not compacted) and ALL rows of a map: the chunk filter
 * `my_chunk % total_chunks == ctg % total_chunks`, the layout, per batch of pieces the decode of templates and reads into an ASCII pool and
 * pgx_cns_pieces' loop at min_cov 1, the stitch (the last 1,000 bytes of a segment against the first 1,050 of the next at band 400, no
 * strings) and the FASTA, all on the device between the upload of the rows and the download of the text.  ctg_names / ctg_name_off: the
 * contigs' names by contig id, name c at [ctg_name_off[c], ctg_name_off[c + 1]), n_names + 1 offsets, n_names beyond the largest contig id.
 * *text (pgx_free): `>name\n bytes \n` per contig in the order of first appearance; *ctg_off (pgx_free): *n_ctg + 1 offsets of the
 * contigs' records in it.  PGX_EINVAL, beyond the layout's refusals: total_chunks == 0, a read the idx lacks, a stitch whose first
 * segment is shorter than 1,000 bytes or whose second is shorter than 1,050, and the refusals of pgx_cns_pieces and of the call, with the
 * contig and the segment named.  PGX_CNS_JOB_BATCH=<pieces per batch>: a test hook. */
int pgx_cns_job_resident(pgx_seqdb *reads, pgx_seqdb *ref, const int64_t *rows, size_t n_rows, uint32_t total_chunks, uint32_t my_chunk,
                         const char *ctg_names, const uint64_t *ctg_name_off, size_t n_names, char **text, uint64_t **ctg_off, uint64_t *n_ctg,
                         uint64_t *text_len, pgx_cns_job_stats *stats);
/* the file level, `pg_asm_cns.py read_db_prefix ref_db_prefix read_to_contig_map total_chunks my_chunk`: <prefix>.idx / .seqdb of both
 * databases and the map file in (parsed on the device in bounded pieces of the file; blanks are what Python's split() takes for one), the
 * script's stdout to out_path (NULL: stdout).  PGX_EINVAL also for the first line that does not hold nine decimal integers that fit. */
int pgx_cns_job(const char *read_db_prefix, const char *ref_db_prefix, const char *map_path, uint32_t total_chunks, uint32_t my_chunk,
                const char *out_path, pgx_cns_job_stats *stats);

/* host utility: the order in which klib khash (src/khash.h:232-336, integer hash :373) iterates n DISTINCT 64-bit keys
 * inserted in the given order -- the order shmr_overlap visits its tables in (src/shmr_overlap.c:206-215).  out receives
 * the n keys in ascending slot order.  Runs on the host (it is the routine the overlap stage uses for its outer table). */
int pgx_khash_slot_order(const uint64_t *keys, size_t n, uint64_t *out);
/* the same with a trailing put of a present key (touch != 0: it only runs the load check, src/khash.h:298-306, and may resize once
 * more).  (Round 3 also offered a device form of this routine -- priority insertion + a fixed point over the eviction order of a
 * resize; exact, and 90x slower than one host thread on the reference's keys, whose constant span byte makes 1 / 256 of the slots
 * the home of every key: removed in round 4) */
int pgx_khash_slot_order_ex(const uint64_t *keys, size_t n, int touch, uint64_t *out);

/* ---- shimmer chain alignment: shmr_aln (src/shmr_align.c:21-160) for a batch of list pairs.  For a pair (list 0, list 1) the shared
 * shimmers are chained into co-linear runs: list 1 is walked in order; a shimmer whose hash x >> 8 list 0 lacks, or holds more than
 * max_repeat times, is skipped; each occurrence in list 0 (in list order) on the same strand is a candidate, appended to the chain opened
 * so far whose last element lies at or before it in list 0, closer than max_dist in list 0's positions, with the smallest change of the
 * offset |pos0 - pos1| below max_diff (the first such chain among equals), or opens a chain.  The walk ends after a shimmer whose last scan
 * saw more than 4,800 chains of fewer than 3 elements (MAX_SMALL_ALNS).  DESIGN.md section 4.9 states the rule in full.
 *   mm0 / off0 / n_lists0 : the lists of side 0 back to back, list l at mm0[off0[l] .. off0[l + 1]) (n_lists0 + 1 offsets from 0); side 1 alike.
 *                           A list of side 0 is indexed once, however many pairs name it.
 *   pairs                 : n_pairs pairs (list of side 0, list of side 1).
 *   *pair_off, *chain_off, *idx0, *idx1 (each the caller's, pgx_free): pair p owns the chains [pair_off[p], pair_off[p + 1]) in the order
 *                           the reference opens them, chain c the elements [chain_off[c], chain_off[c + 1]) in the order it pushes them,
 *                           element e = (idx0[e], idx1[e]), indices into the pair's two lists.  n_pairs + 1 and n_chains + 1 offsets.
 * PGX_ESTATE without pgx_init; PGX_EARG for a null argument, a pair that names a list out of range, offsets that do not start at 0 or
 * decrease, a list (or a side) of 2^31 entries and more, and for direction != 0: the reference's reversed walk begins by reading
 * mmers1->a[n], one past the list, so it has no answer to reproduce.  PGX_ENOMEM leaves nothing allocated.  After any failure the four
 * outputs are untouched.  PGX_SHMR_ALN_LDS=<chains>: a test hook, the chains whose state the walk keeps in LDS (default and most 1024).
 * Device memory is booked as "shmr_aln". ---- */
typedef struct { uint32_t list0, list1; } pgx_shmr_aln_pair;
typedef struct {
  uint64_t n_pairs, n_lists0, n_candidates, n_chains, n_elems, n_stopped;   /* n_candidates: the bound the state was sized by; n_stopped: pairs ended by the small-chain count */
  double gpu_ms, index_ms, walk_ms, unroll_ms;   /* host clock: the whole call; upload + index of side 0; bounds + walk; CSR + download */
} pgx_shmr_aln_stats;
int pgx_shmr_aln_batch(const pgx_mm128 *mm0, const uint64_t *off0, size_t n_lists0, const pgx_mm128 *mm1, const uint64_t *off1, size_t n_lists1,
                       const pgx_shmr_aln_pair *pairs, size_t n_pairs, uint8_t direction, uint32_t max_diff, uint32_t max_dist, uint32_t max_repeat,
                       uint64_t **pair_off, uint64_t **chain_off, uint32_t **idx0, uint32_t **idx1, pgx_shmr_aln_stats *stats);

/* ---- shimmer4py surface (py/peregrine/build_shimmer4py.py:8-84), GPU-backed single-call forms ----
 * NOT exported under their own names: shmr_aln / free_shmr_alns (build_shimmer4py.py:64-77; src/shmr_align.c).  Their answer is
 * offered for a batch of list pairs by pgx_shmr_aln_batch (above), chain for chain the reference's; what it hands out is flat arrays
 * released with pgx_free, not the reference's nested kvecs, so the two names themselves stay with the reference's own shimmer4py. */
typedef struct { size_t n, m; pgx_mm128 *a; } mm128_v; /* kvec layout, src/shimmer.h:27-30; .a is malloc'd, caller frees */
typedef pgx_match ovlp_match_t;
void decode_biseq(uint8_t *src, char *seq, size_t len, uint8_t strand);
void encode_biseq(uint8_t *target, char *seq, size_t len);
void mm_sketch(void *km, const char *str, int len, int w, int k, uint32_t rid, int is_hpc, mm128_v *p);
void mm_reduce(mm128_v *in, mm128_v *out, uint8_t rs);
ovlp_match_t *ovlp_match(uint8_t *query_seq, int32_t q_len, uint8_t q_strand, uint8_t *target_seq,
                         int32_t t_len, uint8_t t_strand, int32_t band_tolerance);
void free_ovlp_match(ovlp_match_t *m);
mm128_v read_mmlist(char *fn);
void write_mmlist(char *fn, mm128_v *p);

/* query helpers (src/shimmer4py.c:44-196, cdef py/peregrine/build_shimmer4py.py:44-62).  The map is
 * built on the GPU by build_shimmer_map4py; the three getters are host lookups over its sorted tables.  On failure
 * build_shimmer_map4py leaves every field of *py_mmer NULL (the reference exit(1)s / asserts) and the getters then return
 * nothing.  get_shimmers_for_read returns a VIEW into py_mmer->mmers (do not free); get_shimmer_hits appends to a
 * caller-owned kvec whose .a is realloc'd (free it with free / pgx_free). */
typedef struct { uint64_t x0, x1, y0, y1; uint8_t direction; } mp256_t;   /* src/shimmer.h:122-126 */
typedef struct { size_t n, m; mp256_t *a; } mp256_v;
typedef struct { mm128_v *mmers; void *mmer0_map; void *rlmap; void *mcmap; void *ridmm; } py_mmer_t; /* shimmer.h:132-138 */
void build_shimmer_map4py(py_mmer_t *py_mmer, char *seqdb_prefix, char *shimmer_prefix, uint32_t mychunk,
                          uint32_t total_chunk, uint32_t lowerbound, uint32_t upperbound);
void get_shimmers_for_read(mm128_v *out, py_mmer_t *py_mmer, uint32_t rid);
uint32_t get_mmer_count(py_mmer_t *py_mmer, uint64_t mhash);
void get_shimmer_hits(mp256_v *out, py_mmer_t *py_mmer, uint64_t mhash0, uint32_t span);
void pgx_shimmer_map_free(py_mmer_t *py_mmer); /* extension: the reference never releases the map */

#ifdef __cplusplus
}
#endif
#endif
