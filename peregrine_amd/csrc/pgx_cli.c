/*
 * pgx_cli.c -- native drop-ins for the reference's stage executables, one multi-call binary (the tool is chosen by the
 * name it is invoked under): shmr_mkseqdb, shmr_index, shmr_overlap, shmr_dedup, shmr_map, shmr_map_merge, path_to_contig.py, graph_to_path.py, pg_asm_cns.py.  Same getopt strings, defaults
 * and output files / streams as /root/reference/src/shmr_mkseqdb.c:14-128, shmr_index.c:37-245, shmr_overlap.c:233-419,
 * shmr_dedup.c:19-104, shmr_map.c:163-373; everything else happens behind the C-ABI of include/pgx.h on the GPU.
 * Plain C against libpgx.so: this is the cgo / FFI-free form of the boundary (the Python shims in bin/ do the same).
 *
 * Resident mode (round 4): `pgx_cli serve -p <seqdb_prefix>` loads the read database into HBM ONCE and then serves shmr_index /
 * shmr_overlap commands for that prefix over a UNIX socket (<seqdb_prefix>.pgx.sock, mode 0600).  The drop-ins look for that socket
 * first: if a server for their -p prefix answers -- and the .seqdb file is still the one it loaded (size + mtime) -- the command runs
 * there (pgx_index_chunk_db / pgx_overlap_chunk_db: same files written, same exit status) and the process start, HIP context and
 * 93 GB upload that each of pg_run.py's 8 + 8 chunk commands would pay are paid once per job.  No socket, a stale one, a different
 * file: the drop-in runs stand-alone as before.  PGX_NO_SERVER=1 never attaches.
 */
#include <errno.h>
#include <libgen.h>
#include <pthread.h>
#include <limits.h>
#include <signal.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/socket.h>
#include <sys/stat.h>
#include <sys/time.h>
#include <sys/un.h>
#include <unistd.h>

#include "../../include/pgx.h"

static int fail(const char *tool, const char *what) {
  fprintf(stderr, "%s: %s failed: %s\n", tool, what, pgx_last_error());
  return 1;
}

static int device_of_env(void) {
  const char *d = getenv("PGX_DEVICE");
  if (d) return atoi(d);
  const char *lr = getenv("LOCAL_RANK");
  return lr ? atoi(lr) : 0;
}

/* ---- resident mode: wire format = one request per connection: "<tool>\0<cwd>\0<size>\0<mtime_ns>\0<argc>\0<argv0>\0...";
 * reply = "<exit status>\0<text for stderr>" ------------------------------------------------------------------------------------ */
static void sock_path_of(const char *prefix, char *out, size_t cap) { snprintf(out, cap, "%s.pgx.sock", prefix); }
static int seqdb_identity(const char *prefix, long long *size, long long *mtime_ns) {
  char path[PATH_MAX];
  struct stat sb;
  snprintf(path, sizeof(path), "%s.seqdb", prefix);
  if (stat(path, &sb)) return -1;
  *size = (long long)sb.st_size;
  *mtime_ns = (long long)sb.st_mtim.tv_sec * 1000000000LL + sb.st_mtim.tv_nsec;
  return 0;
}
static int write_all(int fd, const char *b, size_t n) {
  while (n) {
    const ssize_t w = write(fd, b, n);
    if (w < 0 && errno == EINTR) continue;
    if (w <= 0) return -1;
    b += w, n -= (size_t)w;
  }
  return 0;
}
/* client side: 0..255 = the served command's exit status; -1 = no server took it (run stand-alone) */
static int try_server(const char *tool, const char *prefix, int argc, char **argv) {
  if (getenv("PGX_NO_SERVER")) return -1;
  struct sockaddr_un sa;
  char sp[PATH_MAX];
  sock_path_of(prefix, sp, sizeof(sp));
  if (strlen(sp) >= sizeof(sa.sun_path) || access(sp, F_OK)) return -1;
  long long size = 0, mt = 0;
  if (seqdb_identity(prefix, &size, &mt)) return -1;
  const int fd = socket(AF_UNIX, SOCK_STREAM, 0);
  if (fd < 0) return -1;
  memset(&sa, 0, sizeof(sa));
  sa.sun_family = AF_UNIX;
  strcpy(sa.sun_path, sp);
  if (connect(fd, (struct sockaddr *)&sa, sizeof(sa))) {   /* (blocks while the server's backlog is full: a queued command WAITS, it does not
                                                             * fall back to a stand-alone run beside the server) */
    close(fd);
    return -1;
  }
  {
    struct timeval io = {10, 0};   /* (the request must go out promptly; the reply takes as long as the stage does) */
    (void)setsockopt(fd, SOL_SOCKET, SO_SNDTIMEO, &io, sizeof(io));
  }
  char cwd[PATH_MAX], num[64];
  if (!getcwd(cwd, sizeof(cwd))) cwd[0] = 0;
  int ok = !write_all(fd, tool, strlen(tool) + 1) && !write_all(fd, cwd, strlen(cwd) + 1);
  snprintf(num, sizeof(num), "%lld", size), ok = ok && !write_all(fd, num, strlen(num) + 1);
  snprintf(num, sizeof(num), "%lld", mt), ok = ok && !write_all(fd, num, strlen(num) + 1);
  snprintf(num, sizeof(num), "%d", argc), ok = ok && !write_all(fd, num, strlen(num) + 1);
  for (int i = 0; ok && i < argc; ++i) ok = !write_all(fd, argv[i], strlen(argv[i]) + 1);
  shutdown(fd, SHUT_WR);
  char reply[8192];
  size_t got = 0;
  for (;;) {
    const ssize_t r = read(fd, reply + got, sizeof(reply) - 1 - got);
    if (r < 0 && errno == EINTR) continue;
    if (r <= 0) break;
    got += (size_t)r;
    if (got == sizeof(reply) - 1) break;
  }
  close(fd);
  reply[got] = 0;
  if (!ok || got < 2) return -1;
  const int status = atoi(reply);
  if (status == 250) return -1; /* the server declined (another file behind that prefix now): stand-alone */
  const char *text = reply + strlen(reply) + 1;
  if (text < reply + got && *text) fputs(text, stderr);
  return status;
}

/* An output the SERVER cannot open on the client's behalf: /dev/stdout, /dev/fd/N, /proc/self/fd/N (process substitution) name
 * the calling process's descriptors, and anything that exists and is not a regular file (a FIFO, a socket, a tty) may mean something else over
 * there too.  Such a command runs stand-alone, where fopen(path) does what the reference's does (src/shmr_overlap.c:341-352). */
static int output_needs_this_process(const char *path) {
  if (!path) return 0;
  if (!strncmp(path, "/dev/std", 8) || !strncmp(path, "/dev/fd/", 8) || !strncmp(path, "/dev/tty", 8) || !strncmp(path, "/proc/", 6)) return 1;   /* (not /dev/shm/...: plain files) */
  struct stat sb;
  if (stat(path, &sb) == 0 && !S_ISREG(sb.st_mode)) return 1;
  return 0;
}

static int run_index_args(int argc, char **argv, pgx_seqdb *db, const char *served_prefix, char *msg, size_t cap);
static int run_overlap_args(int argc, char **argv, pgx_seqdb *db, const char *served_prefix, char *msg, size_t cap, pgx_output **pending);

static void send_reply(int fd, int status, const char *msg) {
  char head[16];
  snprintf(head, sizeof(head), "%d", status);
  if (!write_all(fd, head, strlen(head) + 1)) (void)write_all(fd, msg, strlen(msg) + 1);
  close(fd);
}
/* A served overlap command whose GPU stage is done: its output file is completed (pgx_output_finish) and its client answered on a thread of
 * its own, while the server's loop already runs the next command's stage (round 6). */
struct finisher {
  int fd, status;
  pgx_output *pending;
  char msg[4096];
};
static void *finish_and_reply(void *arg) {
  struct finisher *f = (struct finisher *)arg;
  if (pgx_output_finish(f->pending)) {
    const size_t n = strlen(f->msg);
    snprintf(f->msg + n, sizeof(f->msg) - n, "shmr_overlap: pgx_output_finish failed: %s\n", pgx_last_error());
    f->status = 1;
  }
  send_reply(f->fd, f->status, f->msg);
  free(f);
  return NULL;
}

static volatile sig_atomic_t g_stop = 0;
static char g_sock[PATH_MAX];
static void on_term(int sig) {
  (void)sig;
  g_stop = 1;
  if (g_sock[0]) unlink(g_sock);
  _exit(0);
}
static int main_serve(int argc, char **argv) {
  const char *prefix = "seq_dataset";
  int c, idle_s = 0;
  while ((c = getopt(argc, argv, "p:i:")) != -1) {
    if (c == 'p') prefix = optarg;
    else if (c == 'i') idle_s = atoi(optarg); /* leave after that many seconds without a request (0: never) */
    else {
      fprintf(stderr, "Usage: pgx_cli serve -p seqdb_prefix [-i idle_seconds]\n");
      return 1;
    }
  }
  long long size = 0, mt = 0;
  if (seqdb_identity(prefix, &size, &mt)) {
    fprintf(stderr, "pgx_cli serve: %s.seqdb: %s\n", prefix, strerror(errno));
    return 1;
  }
  if (pgx_init(device_of_env())) return fail("pgx_cli serve", "pgx_init");
  pgx_seqdb *db = NULL;
  if (pgx_seqdb_load(prefix, &db)) return fail("pgx_cli serve", "pgx_seqdb_load");
  struct sockaddr_un sa;
  sock_path_of(prefix, g_sock, sizeof(g_sock));
  if (strlen(g_sock) >= sizeof(sa.sun_path)) {
    fprintf(stderr, "pgx_cli serve: socket path too long: %s\n", g_sock);
    return 1;
  }
  unlink(g_sock);
  const int ls = socket(AF_UNIX, SOCK_STREAM, 0);
  memset(&sa, 0, sizeof(sa));
  sa.sun_family = AF_UNIX;
  strcpy(sa.sun_path, g_sock);
  const mode_t old = umask(0177);
  if (ls < 0 || bind(ls, (struct sockaddr *)&sa, sizeof(sa)) || listen(ls, 64)) {
    fprintf(stderr, "pgx_cli serve: cannot listen on %s: %s\n", g_sock, strerror(errno));
    return 1;
  }
  umask(old);
  signal(SIGTERM, on_term), signal(SIGINT, on_term), signal(SIGPIPE, SIG_IGN);
  fprintf(stderr, "pgx_cli serve: %s.seqdb (%llu reads, %llu bases) resident on GPU %d; serving %s\n", prefix, (unsigned long long)pgx_seqdb_reads(db),
          (unsigned long long)pgx_seqdb_bases(db), device_of_env(), g_sock);
  while (!g_stop) {
    if (idle_s > 0) {
      fd_set rf;
      struct timeval tv = {idle_s, 0};
      FD_ZERO(&rf);
      FD_SET(ls, &rf);
      if (select(ls + 1, &rf, NULL, NULL, &tv) == 0) break;
    }
    const int fd = accept(ls, NULL, NULL);
    if (fd < 0) {
      if (errno == EINTR) continue;
      break;
    }
    {  /* a stalled or half-open client must not hold every later command of the job: the request is a few hundred bytes */
      struct timeval io = {10, 0};
      (void)setsockopt(fd, SOL_SOCKET, SO_RCVTIMEO, &io, sizeof(io));
      (void)setsockopt(fd, SOL_SOCKET, SO_SNDTIMEO, &io, sizeof(io));
    }
    static char req[1 << 16];
    size_t got = 0;
    for (;;) {
      const ssize_t r = read(fd, req + got, sizeof(req) - 1 - got);
      if (r < 0 && errno == EINTR) continue;
      if (r <= 0) break;
      got += (size_t)r;
      if (got == sizeof(req) - 1) break;
    }
    req[got] = 0;
    /* split at the NULs */
    char *fld[520];
    int nf = 0;
    for (size_t o = 0; o < got && nf < 520; o += strlen(req + o) + 1) fld[nf++] = req + o;
    char msg[4096];
    msg[0] = 0;
    int status = 250;
    pgx_output *pending = NULL;
    if (nf >= 5) {
      const char *tool = fld[0], *cwd = fld[1];
      const long long csize = atoll(fld[2]), cmt = atoll(fld[3]);
      const int ac = atoi(fld[4]);
      long long nsize = 0, nmt = 0;
      if (ac >= 1 && 5 + ac <= nf && csize == size && cmt == mt && !seqdb_identity(prefix, &nsize, &nmt) && nsize == size && nmt == mt) {
        char here[PATH_MAX];
        if (!getcwd(here, sizeof(here))) here[0] = 0;
        if (cwd[0] && chdir(cwd)) snprintf(msg, sizeof(msg), "pgx_cli serve: cannot enter %s\n", cwd), status = 1;
        else {
          optind = 0; /* (glibc: 0 re-initialises getopt completely, also after a scan that stopped inside a clustered option) */
          if (!strcmp(tool, "shmr_index")) status = run_index_args(ac, fld + 5, db, prefix, msg, sizeof(msg));
          else if (!strcmp(tool, "shmr_overlap")) status = run_overlap_args(ac, fld + 5, db, prefix, msg, sizeof(msg), &pending);
          if (here[0] && chdir(here)) status = status ? status : 1;
        }
      }
    }
    if (pending) {   /* the records are still on their way to the file: finish + reply on a thread, the loop takes the next command */
      struct finisher *f = (struct finisher *)malloc(sizeof(*f));
      pthread_t th;
      pthread_attr_t at;
      pthread_attr_init(&at);
      pthread_attr_setdetachstate(&at, PTHREAD_CREATE_DETACHED);
      if (f) f->fd = fd, f->status = status, f->pending = pending, snprintf(f->msg, sizeof(f->msg), "%s", msg);
      if (!f || pthread_create(&th, &at, finish_and_reply, f)) {   /* no thread: the same inline */
        if (pgx_output_finish(pending)) status = 1;
        free(f);
        send_reply(fd, status, msg);
      }
      pthread_attr_destroy(&at);
    } else {
      send_reply(fd, status, msg);
    }
  }
  unlink(g_sock);
  pgx_seqdb_free(db);
  return 0;
}

static int main_mkseqdb(int argc, char **argv) {
  const char *list = "seq_dataset.lst", *prefix = "seq_dataset";
  int c;
  while ((c = getopt(argc, argv, "d:p:")) != -1) {
    if (c == 'd') list = optarg;
    else if (c == 'p') prefix = optarg;
    else {
      fprintf(stderr, "Usage: shmr_mkseqdb -d seq_dataset.lst -p seq_dataset_prefix\n");
      return 1;
    }
  }
  printf("input sequence dataset file list: '%s'\noutput index file: %s.idx\noutput seqdb file: %s.idx\n", list, prefix, prefix);
  if (pgx_init(device_of_env())) return fail("shmr_mkseqdb", "pgx_init");
  uint64_t nr = 0, nb = 0;
  if (pgx_mkseqdb(list, prefix, &nr, &nb)) return fail("shmr_mkseqdb", "pgx_mkseqdb");
  return 0;
}

/* db != NULL: the served form (the database of served_prefix is resident); messages go to msg instead of stderr */
static int run_index_args(int argc, char **argv, pgx_seqdb *db, const char *served_prefix, char *msg, size_t cap) {
  const char *p = "seq_dataset", *o = "shimmer";
  pgx_index_params ip = {1, 1, 2, 6, 80, 16, 1}; /* -t -c -l -r -w -k -m : shmr_index.c:21-23,49-55 */
  int c, m = 1, hpc = 0; /* -H: homopolymer-compressed shimmers (minimap2's letter; free in the reference's getopt string) */
  while ((c = getopt(argc, argv, "p:o:t:c:l:r:m:w:k:H")) != -1) {
    switch (c) {
      case 'p': p = optarg; break;
      case 'o': o = optarg; break;
      case 't': ip.total_chunk = atoi(optarg); break;
      case 'c': ip.mychunk = atoi(optarg); break;
      case 'l': ip.levels = atoi(optarg); break;
      case 'r': ip.reduction = atoi(optarg); break;
      case 'm': m = atoi(optarg); break;
      case 'H': hpc = 1; break;
      case 'w': ip.window = atoi(optarg); break;
      case 'k': ip.kmer = atoi(optarg); break;
      default: return 1; /* the reference returns 1 on a missing option argument (:93-107) */
    }
  }
  ip.want_l0 = (m == 1 ? 1 : m ? 2 : 0) | (hpc ? PGX_INDEX_HPC : 0); /* (only 1 writes L0 files: shmr_index.c:165; another number: no fused path) */
  if (!db) {
    const int served = try_server("shmr_index", p, argc, argv);
    if (served >= 0) return served;
    fprintf(stderr, "reduction factor= %d\nusing index file: %s.idx\nusing seqdb file: %s.seqdb\n", ip.reduction, p, p);
    if (pgx_init(device_of_env())) return fail("shmr_index", "pgx_init");
    if (pgx_index_chunk(p, o, &ip, NULL)) return fail("shmr_index", "pgx_index_chunk");
    return 0;
  }
  if (strcmp(p, served_prefix)) return 250; /* not the database this server holds */
  int n = snprintf(msg, cap, "reduction factor= %d\nusing index file: %s.idx\nusing seqdb file: %s.seqdb (resident: pgx_cli serve)\n", ip.reduction, p, p);
  if (pgx_index_chunk_db(db, o, &ip, NULL)) {
    snprintf(msg + n, cap - (size_t)n, "shmr_index: pgx_index_chunk_db failed: %s\n", pgx_last_error());
    return 1;
  }
  return 0;
}
static int main_index(int argc, char **argv) { return run_index_args(argc, argv, NULL, NULL, NULL, 0); }

static int run_overlap_args(int argc, char **argv, pgx_seqdb *db, const char *served_prefix, char *msg, size_t cap, pgx_output **pending) {
  const char *p = "seq_dataset", *l = "shimmer-L2", *o = NULL;
  pgx_overlap_params op = {1, 1, 4, 2, 240, 100, 120}; /* -t -c -b -m -M -w -n : shmr_overlap.c:28-42,245-251 */
  char dflt[64];
  int c;
  while ((c = getopt(argc, argv, "p:l:t:c:b:o:m:M:w:n:")) != -1) {
    switch (c) {
      case 'p': p = optarg; break;
      case 'l': l = optarg; break;
      case 'o': o = optarg; break;
      case 't': op.total_chunk = atoi(optarg); break;
      case 'c': op.mychunk = atoi(optarg); break;
      case 'b': op.bestn = atoi(optarg); break;
      case 'm': op.mc_lower = atoi(optarg); break;
      case 'M': op.mc_upper = atoi(optarg); break;
      case 'w': op.align_bandwidth = atoi(optarg); break;
      case 'n': op.ovlp_upper = atoi(optarg); break;
      default: return 1;
    }
  }
  if (!o) { /* :341-344 */
    snprintf(dflt, sizeof(dflt), "ovlp.%02d", op.mychunk);
    o = dflt;
  }
  if (!db) {
    const int served = output_needs_this_process(o) ? -1 : try_server("shmr_overlap", p, argc, argv);
    if (served >= 0) return served;
    if (pgx_init(device_of_env())) return fail("shmr_overlap", "pgx_init");
    if (pgx_overlap_chunk(p, l, o, &op, NULL)) return fail("shmr_overlap", "pgx_overlap_chunk");
    return 0;
  }
  if (strcmp(p, served_prefix)) return 250;
  if (pgx_overlap_chunk_db_begin(db, l, o, &op, NULL, pending)) {   /* (the caller finishes the output: pgx_output_finish) */
    snprintf(msg, cap, "shmr_overlap: pgx_overlap_chunk_db failed: %s\n", pgx_last_error());
    return 1;
  }
  return 0;
}
static int main_overlap(int argc, char **argv) { return run_overlap_args(argc, argv, NULL, NULL, NULL, 0, NULL); }

/* shmr_dedup: the ovlp_t stream from stdin (cat ovlp*.dat | shmr_dedup, pg_run.py:351-352) goes through a pgx_dedup stream in pieces of
 * PGX_DEDUP_PIECE records (default 16 Mi = 1 GiB; a test hook).  Two piece buffers: a reader thread fills one while the GPU works on the
 * other, and each feed's text is written as it comes back -- host memory is two pieces and about two copies of one feed's text whatever
 * the stream's length.
 * -g (the reference's tool takes no flags): a graph-mode stream -- nothing is written until the end of stdin, then the lines the string
 * graph's loader uses are drained in pieces of PGX_DEDUP_PIECE lines. */
struct dedup_reader {
  char *buf;
  size_t cap, got;   /* bytes; cap is a whole number of records */
};
static void *dedup_read_piece(void *arg) {
  struct dedup_reader *r = (struct dedup_reader *)arg;
  size_t n = 0;
  while (n < r->cap) {   /* (a pipe returns short counts: only the end of the stream leaves a piece short) */
    const size_t got = fread(r->buf + n, 1, r->cap - n, stdin);
    if (got == 0) break;
    n += got;
  }
  r->got = n;
  return NULL;
}
/* stdin through a dedup stream piece by piece.  graph: a graph-mode stream, whose lines come after the end of the input; sg != NULL: instead
 * of those lines the string graph of them, as the sg_edges_list text (shmr_sgraph) */
struct sgraph_opts {
  long long min_len;
  double min_idt;
  const char *utg;   /* --utg FILE: the unitigs' lines go there (NULL: none are made) */
  const char *utg_data, *ctg_paths;   /* --utg-data FILE, --ctg-paths FILE: the final utg_data and ctg_paths (NULL: not written) */
  int chimer_ordered;                 /* --chimer_bridge_ordered: PGX_SGRAPH_CHIMER_ORDERED */
  const char *chimers_nodes;          /* --chimers-nodes FILE: the chimers_nodes file (NULL: not written) */
  const char *gfa, *gfa_seqdb;        /* --gfa FILE: the unitig graph as GFA; --gfa-seqdb PREFIX: with the sequences from that database */
};
/* What every hand-out of text ends with: the status of the call `what` reported, or its text written to f (named fname in the
 * complaint); the text is freed either way.  Returns the exit code so far. */
static int put_text(const char *tool, const char *what, int status, char *text, size_t len, FILE *f, const char *fname) {
  int rc = 0;
  if (status) rc = fail(tool, what);
  else if (fwrite(text, 1, len, f) != len) rc = 1, perror(fname);
  pgx_free(text);
  return rc;
}
/* the three hand-outs that go piece by piece, with one signature (obj: the handle) */
typedef int (*next_text_fn)(void *obj, uint64_t max_lines, char **text, size_t *len, int *done);
static int next_sgraph_text(void *g, uint64_t n, char **text, size_t *len, int *done) { return pgx_sgraph_text((pgx_sgraph *)g, n, text, len, done); }
static int next_unitigs_text(void *u, uint64_t n, char **text, size_t *len, int *done) { return pgx_unitigs_text((pgx_unitigs *)u, n, text, len, done); }
static int next_ctg_utg_text(void *c, uint64_t n, char **text, size_t *len, int *done) { return pgx_ctg_paths_utg_text((pgx_ctg_paths *)c, n, text, len, done); }
static int next_ctg_ctg_text(void *c, uint64_t n, char **text, size_t *len, int *done) { return pgx_ctg_paths_ctg_text((pgx_ctg_paths *)c, n, text, len, done); }
static int next_drain_text(void *s, uint64_t n, char **text, size_t *len, int *done) { return pgx_dedup_drain((pgx_dedup_stream *)s, n, text, len, done); }
/* all the text obj still has, in pieces of `piece` lines, to f */
static int write_pieces(const char *tool, const char *what, next_text_fn next, void *obj, size_t piece, FILE *f, const char *fname) {
  for (int done = 0; !done;) {
    char *text = NULL;
    size_t len = 0;
    const int status = next(obj, piece, &text, &len, &done);
    const int rc = put_text(tool, what, status, text, len, f, fname);
    if (rc) return rc;
  }
  return 0;
}
/* all the text of obj to the file at path */
static int write_text_file(const char *tool, const char *what, next_text_fn next, void *obj, size_t piece, const char *path) {
  FILE *f = fopen(path, "wb");
  if (!f) {
    perror(path);
    return 1;
  }
  int rc = write_pieces(tool, what, next, obj, piece, f, path);
  if (fclose(f) && !rc) rc = 1, perror(path);
  return rc;
}
/* the unitigs of g: their lines to sg->utg, the final utg_data and ctg_paths made of them to sg->utg_data and sg->ctg_paths (each if named) */
static int write_unitigs(const char *tool, pgx_sgraph *g, const struct sgraph_opts *sg, size_t piece) {
  pgx_unitigs *u = NULL;
  pgx_ctg_paths *c = NULL;
  int rc = 0;
  if (pgx_sgraph_unitigs(g, &u)) rc = fail(tool, "pgx_sgraph_unitigs");
  if (!rc && sg->gfa) {   /* nothing is written unless the whole graph was built */
    pgx_gfa *f = NULL;
    if (pgx_gfa_build_files(u, g, NULL, 0, sg->gfa_seqdb, &f)) rc = fail(tool, "pgx_gfa_build_files");
    else if (pgx_gfa_write(f, sg->gfa)) rc = fail(tool, "pgx_gfa_write");
    pgx_gfa_free(f);
  }
  if (!rc && sg->utg) rc = write_text_file(tool, "pgx_unitigs_text", next_unitigs_text, u, piece, sg->utg);
  if (!rc && (sg->utg_data || sg->ctg_paths) && pgx_unitigs_contig_paths(u, &c)) rc = fail(tool, "pgx_unitigs_contig_paths");
  if (!rc && sg->utg_data) rc = write_text_file(tool, "pgx_ctg_paths_utg_text", next_ctg_utg_text, c, piece, sg->utg_data);
  if (!rc && sg->ctg_paths) rc = write_text_file(tool, "pgx_ctg_paths_ctg_text", next_ctg_ctg_text, c, piece, sg->ctg_paths);
  pgx_ctg_paths_free(c);
  pgx_unitigs_free(u);
  return rc;
}
/* the chimers_nodes file of g to the file at path */
static int write_chimers_nodes(const char *tool, const pgx_sgraph *g, const char *path) {
  FILE *f = fopen(path, "wb");
  if (!f) {
    perror(path);
    return 1;
  }
  char *text = NULL;
  size_t len = 0;
  const int status = pgx_sgraph_chimer_nodes(g, &text, &len);
  int rc = put_text(tool, "pgx_sgraph_chimer_nodes", status, text, len, f, path);
  if (fclose(f) && !rc) rc = 1, perror(path);
  return rc;
}
static int dedup_stdin(const char *tool, int graph, const struct sgraph_opts *sg) {
  size_t piece = (size_t)16 << 20;
  const char *pe = getenv("PGX_DEDUP_PIECE");
  if (pe && atoll(pe) > 0) piece = (size_t)atoll(pe);
  if (piece >= ((size_t)1 << 31)) piece = ((size_t)1 << 31) - 1;
  char *bufs[2] = {(char *)malloc(piece * sizeof(pgx_ovlp)), (char *)malloc(piece * sizeof(pgx_ovlp))};
  if (!bufs[0] || !bufs[1]) {
    fprintf(stderr, "%s: out of host memory\n", tool);
    return 1;
  }
  struct dedup_reader rd = {bufs[0], piece * sizeof(pgx_ovlp), 0};
  pthread_t th;
  if (pthread_create(&th, NULL, dedup_read_piece, &rd)) {   /* the first piece is read while the device context comes up */
    fprintf(stderr, "%s: cannot start the reader thread\n", tool);
    free(bufs[0]), free(bufs[1]);
    return 1;
  }
  pgx_dedup_stream *ds = NULL;
  int rc = 0, open_failed = 0;
  if (pgx_init(device_of_env())) rc = fail(tool, "pgx_init"), open_failed = 1;
  else if (graph ? pgx_dedup_open_graph(0, &ds) : pgx_dedup_open(0, &ds)) rc = fail(tool, "pgx_dedup_open"), open_failed = 1;
  for (int k = 0;; k ^= 1) {
    pthread_join(th, NULL);
    const size_t got = rd.got;
    if (got < sizeof(pgx_ovlp) || open_failed) break;
    rd.buf = bufs[k ^ 1];
    const int more = got == rd.cap;   /* a short piece was the last one (a trailing partial record is dropped, as today) */
    if (more && pthread_create(&th, NULL, dedup_read_piece, &rd)) {
      fprintf(stderr, "%s: cannot start the reader thread\n", tool);
      rc = 1;
      break;
    }
    char *text = NULL;
    size_t len = 0;
    const int status = pgx_dedup_feed(ds, (const pgx_ovlp *)bufs[k], got / sizeof(pgx_ovlp), &text, &len);
    rc = put_text(tool, "pgx_dedup_feed", status, text, len, stdout, "stdout");
    if (rc) {
      if (more) pthread_join(th, NULL);
      break;
    }
    if (!more) break;
  }
  pgx_sgraph *g = NULL;
  if (sg && ds && !rc && pgx_sgraph_build(ds, sg->min_len, sg->min_idt, sg->chimer_ordered ? PGX_SGRAPH_CHIMER_ORDERED : 0, &g)) rc = fail(tool, "pgx_sgraph_build");
  if (g) rc = write_pieces(tool, "pgx_sgraph_text", next_sgraph_text, g, piece, stdout, "stdout");
  if (g && sg->chimers_nodes && !rc) rc = write_chimers_nodes(tool, g, sg->chimers_nodes);
  if (g && (sg->utg || sg->utg_data || sg->ctg_paths || sg->gfa) && !rc) rc = write_unitigs(tool, g, sg, piece);
  pgx_sgraph_free(g);
  if (graph && !sg && ds && !rc) rc = write_pieces(tool, "pgx_dedup_drain", next_drain_text, ds, piece, stdout, "stdout");
  if (ds) pgx_dedup_close(ds, NULL, NULL);
  free(bufs[0]), free(bufs[1]);
  return rc;
}

static int main_dedup(int argc, char **argv) {
  int graph = 0;
  for (int i = 1; i < argc; ++i) graph |= strcmp(argv[i], "-g") == 0;   /* (other arguments are ignored, as ever) */
  return dedup_stdin("shmr_dedup", graph, NULL);
}

/* cat ovlp*.dat | shmr_sgraph [--min_len N] [--min_idt X] [--utg FILE] [--utg-data FILE] [--ctg-paths FILE] [--gfa FILE [--gfa-seqdb PREFIX]] > sg_edges_list: the first half of ovlp_to_graph.py (its defaults), with
 * --disable_chimer_bridge_removal and without --lfc; --chimer_bridge_ordered [--chimers-nodes FILE] runs the chimer bridge step too, under the
 * stated pop order (pgx.h, PGX_SGRAPH_CHIMER_ORDERED) */
static int main_sgraph(int argc, char **argv) {
  struct sgraph_opts o = {4000, 96.0, NULL, NULL, NULL, 0, NULL, NULL, NULL};
  for (int i = 1; i < argc; ++i) {
    const char *a = argv[i], *v = NULL;
    const int len_opt = strncmp(a, "--min_len", 9) == 0 && (a[9] == 0 || a[9] == '='), idt_opt = strncmp(a, "--min_idt", 9) == 0 && (a[9] == 0 || a[9] == '=');
    if (len_opt || idt_opt) {
      v = a[9] ? a + 10 : (i + 1 < argc ? argv[++i] : NULL);
      char *end = NULL;
      if (v && len_opt) o.min_len = strtoll(v, &end, 10);
      else if (v) o.min_idt = strtod(v, &end);
      if (!v || end == v || *end) {
        fprintf(stderr, "shmr_sgraph: %.9s needs a number\n", a);
        return 2;
      }
    } else if (strncmp(a, "--utg", 5) == 0 && (a[5] == 0 || a[5] == '=')) {
      o.utg = a[5] ? a + 6 : (i + 1 < argc ? argv[++i] : NULL);
      if (!o.utg || !*o.utg) {
        fprintf(stderr, "shmr_sgraph: --utg needs a file name\n");
        return 2;
      }
    } else if ((strncmp(a, "--utg-data", 10) == 0 && (a[10] == 0 || a[10] == '=')) || (strncmp(a, "--ctg-paths", 11) == 0 && (a[11] == 0 || a[11] == '='))) {
      const size_t nl = a[2] == 'u' ? 10 : 11;
      const char **dst = a[2] == 'u' ? &o.utg_data : &o.ctg_paths;
      *dst = a[nl] ? a + nl + 1 : (i + 1 < argc ? argv[++i] : NULL);
      if (!*dst || !**dst) {
        fprintf(stderr, "shmr_sgraph: %.*s needs a file name\n", (int)nl, a);
        return 2;
      }
    } else if ((strncmp(a, "--gfa-seqdb", 11) == 0 && (a[11] == 0 || a[11] == '=')) || (strncmp(a, "--gfa", 5) == 0 && (a[5] == 0 || a[5] == '='))) {
      const size_t nl = a[5] == '-' ? 11 : 5;
      const char **dst = nl == 11 ? &o.gfa_seqdb : &o.gfa;
      *dst = a[nl] ? a + nl + 1 : (i + 1 < argc ? argv[++i] : NULL);
      if (!*dst || !**dst) {
        fprintf(stderr, "shmr_sgraph: %.*s needs a %s\n", (int)nl, a, nl == 11 ? "seqdb prefix" : "file name");
        return 2;
      }
    } else if (strcmp(a, "--chimer_bridge_ordered") == 0) {
      o.chimer_ordered = 1;
    } else if (strncmp(a, "--chimers-nodes", 15) == 0 && (a[15] == 0 || a[15] == '=')) {
      o.chimers_nodes = a[15] ? a + 16 : (i + 1 < argc ? argv[++i] : NULL);
      if (!o.chimers_nodes || !*o.chimers_nodes) {
        fprintf(stderr, "shmr_sgraph: --chimers-nodes needs a file name\n");
        return 2;
      }
    } else if (strcmp(a, "--lfc") == 0) {
      fprintf(stderr, "shmr_sgraph: --lfc is not offered (pg_run.py leaves it off)\n");
      return 2;
    } else if (strcmp(a, "--disable_chimer_bridge_removal") == 0) {
      /* what this tool always does */
    } else if (strcmp(a, "--chimer_bridge_removal") == 0) {
      fprintf(stderr, "shmr_sgraph: the chimer bridge step as the script runs it is not offered (it pops from a set of objects: the script's own output changes "
                      "with the hash seed); --chimer_bridge_ordered runs it under a stated pop order, or compare with ovlp_to_graph.py --disable_chimer_bridge_removal\n");
      return 2;
    } else {
      fprintf(stderr, "usage: shmr_sgraph [--min_len N] [--min_idt X] [--disable_chimer_bridge_removal | --chimer_bridge_ordered [--chimers-nodes FILE]] [--utg FILE] [--utg-data FILE] [--ctg-paths FILE] [--gfa FILE [--gfa-seqdb PREFIX]] < ovlp.dat > sg_edges_list\n");
      return 2;
    }
  }
  if (o.chimers_nodes && !o.chimer_ordered) {
    fprintf(stderr, "shmr_sgraph: --chimers-nodes needs --chimer_bridge_ordered\n");
    return 2;
  }
  if (o.gfa_seqdb && !o.gfa) {
    fprintf(stderr, "shmr_sgraph: --gfa-seqdb needs --gfa\n");
    return 2;
  }
  return dedup_stdin("shmr_sgraph", 1, &o);
}

static int main_map(int argc, char **argv) {
  const char *r = "ref", *m = "ref-L2", *p = "seq_dataset", *l = "shimmer-L2";
  pgx_map_params mp = {1, 1, 1, 240}; /* -t -c -n -M : shmr_map.c:28-29,176-177 */
  int c;
  while ((c = getopt(argc, argv, "r:m:p:l:M:n:t:c:b:")) != -1) {
    switch (c) {
      case 'r': r = optarg; break;
      case 'm': m = optarg; break;
      case 'p': p = optarg; break;
      case 'l': l = optarg; break;
      case 'M': mp.mc_upper = atoi(optarg); break;
      case 'n': mp.mc_lower = atoi(optarg); break;
      case 't': mp.total_chunk = atoi(optarg); break;
      case 'c': mp.mychunk = atoi(optarg); break;
      case 'b': break; /* accepted by the reference's getopt string, never used */
      default: return 1;
    }
  }
  if (pgx_init(device_of_env())) return fail("shmr_map", "pgx_init");
  char *text = NULL;
  size_t len = 0;
  uint64_t nl = 0;
  if (pgx_map_chunk(r, m, p, l, &mp, &text, &len, &nl)) return fail("shmr_map", "pgx_map_chunk");
  fwrite(text, 1, len, stdout);
  pgx_free(text);
  return 0;
}

/* path_to_contig.py <seqdb_prefix> <tiling_path> > contigs.fa (py/scripts/path_to_contig.py; pg_run.py:356-362 runs it for the primary and for
 * the alternate contigs).  Always stand-alone: it uploads only the reads the path names, `pgx_cli serve` is not asked. */
static int main_path_to_contig(int argc, char **argv) {
  if (argc != 3) {
    fprintf(stderr, "Usage: path_to_contig.py seqdb_prefix tiling_path > contigs.fa\n");
    return 1;
  }
  if (pgx_init(device_of_env())) return fail("path_to_contig.py", "pgx_init");
  if (pgx_contigs_chunk(argv[1], argv[2], NULL, NULL, NULL)) return fail("path_to_contig.py", "pgx_contigs_chunk");
  return 0;
}

/* pg_asm_cns.py <read_db_prefix> <ref_db_prefix> <read_to_contig_map> <total_chunks> <my_chunk> > cns.fa (py/scripts/pg_asm_cns.py, the
 * last stage of pg_run.py).  Always stand-alone: both databases are loaded by this process. */
static int parse_chunk(const char *s, uint32_t *out) {
  char *end = NULL;
  errno = 0;
  const long long v = strtoll(s, &end, 10);
  if (errno || end == s || *end || v < 0 || v > 0xFFFFFFFFll) return 0;
  *out = (uint32_t)v;
  return 1;
}
static int main_pg_asm_cns(int argc, char **argv) {
  uint32_t total = 0, my = 0;
  if (argc != 6 || !parse_chunk(argv[4], &total) || !parse_chunk(argv[5], &my)) {
    fprintf(stderr, "Usage: pg_asm_cns.py read_db_prefix ref_db_prefix read_to_contig_map total_chunks my_chunk > cns.fa\n");
    return 1;
  }
  if (pgx_init(device_of_env())) return fail("pg_asm_cns.py", "pgx_init");
  if (pgx_cns_job(argv[1], argv[2], argv[3], total, my, NULL, NULL)) return fail("pg_asm_cns.py", "pgx_cns_job");
  return 0;
}

/* shmr_map_merge [FILE...] [-o OUT]: the map chunk files in the order of `LC_ALL=C sort -k 1 -g -k 2 -g` over their lines, the step between
 * shmr_map and pg_asm_cns.py (pg_run.py:491-496).  Without files it reads stdin, so `cat map-*.dat | shmr_map_merge > out` works too. */
static int main_map_merge(int argc, char **argv) {
  const char *out = NULL, *in_stdin = "-";
  const char **paths = malloc(sizeof(char *) * (size_t)(argc > 1 ? argc : 1));
  size_t n = 0;
  int bad = paths == NULL;
  for (int i = 1; i < argc && !bad; ++i) {
    if (strcmp(argv[i], "-o") == 0) {
      if (i + 1 < argc && !out) out = argv[++i];
      else bad = 1;
    } else if (argv[i][0] == '-' && argv[i][1]) {
      bad = 1;
    } else {
      paths[n++] = argv[i];
    }
  }
  if (bad) {
    fprintf(stderr, "usage: shmr_map_merge [FILE...] [-o OUT]   (no FILE: stdin; no -o: stdout)\n");
    return 1;
  }
  if (n == 0) paths[n++] = in_stdin;
  if (pgx_init(device_of_env())) return fail("shmr_map_merge", "pgx_init");
  if (pgx_map_merge(paths, n, out, NULL)) return fail("shmr_map_merge", "pgx_map_merge");
  return 0;
}

/* graph_to_path.py [--improper-p-ctg] [--proper-a-ctg] [--seqdb-prefix P] [--sg-edges-list-fn F] [--utg-data-fn F] [--ctg-paths-fn F]
 * (py/scripts/graph_to_path.py): p_ctg_tiling_path and a_ctg_tiling_path into the working directory, nothing on stdout.  The first three
 * options change nothing in the script's tiling paths either. */
static int main_graph_to_path(int argc, char **argv) {
  const char *sg = "./sg_edges_list", *utg = "./utg_data", *ctg = "./ctg_paths", *seqdb = "./seq_dataset", *fa[2] = {NULL, NULL};
  for (int i = 1; i < argc; ++i) {
    const char *a = argv[i];
    const char **dst = NULL;
    size_t len = 0;
    if (strcmp(a, "--improper-p-ctg") == 0 || strcmp(a, "--proper-a-ctg") == 0) continue;
    if (strncmp(a, "--seqdb-prefix", len = 14) == 0) dst = &seqdb;
    else if (strncmp(a, "--p-ctg-fa", len = 10) == 0) dst = &fa[0];
    else if (strncmp(a, "--a-ctg-fa", len = 10) == 0) dst = &fa[1];
    else if (strncmp(a, "--sg-edges-list-fn", len = 18) == 0) dst = &sg;
    else if (strncmp(a, "--utg-data-fn", len = 13) == 0) dst = &utg;
    else if (strncmp(a, "--ctg-paths-fn", len = 14) == 0) dst = &ctg;
    if (dst && a[len] == '=') *dst = a + len + 1;
    else if (dst && a[len] == 0 && i + 1 < argc) *dst = argv[++i];
    else {
      fprintf(stderr, "usage: graph_to_path.py [--improper-p-ctg] [--proper-a-ctg] [--seqdb-prefix P] [--sg-edges-list-fn F] [--utg-data-fn F] [--ctg-paths-fn F] [--p-ctg-fa FILE] [--a-ctg-fa FILE]\n");
      return 2;
    }
  }
  if (pgx_init(device_of_env())) return fail("graph_to_path.py", "pgx_init");
  if (!fa[0] && !fa[1]) {
    if (pgx_tiling_chunk(sg, utg, ctg, "p_ctg_tiling_path", "a_ctg_tiling_path", NULL)) return fail("graph_to_path.py", "pgx_tiling_chunk");
    return 0;
  }
  /* with FASTA: the tiling stays alive; both texts are whole in memory before the first file is opened, the contigs come from its rows */
  char *small[2] = {NULL, NULL}, *text[2] = {NULL, NULL};
  size_t small_len[2] = {0, 0}, text_len[2] = {0, 0};
  const char *small_fn[2] = {utg, ctg}, *out_fn[2] = {"p_ctg_tiling_path", "a_ctg_tiling_path"};
  for (int k = 0; k < 2; ++k) {
    FILE *f = fopen(small_fn[k], "rb");
    if (!f) {
      fprintf(stderr, "graph_to_path.py: cannot read %s\n", small_fn[k]);
      return 1;
    }
    size_t cap = 1 << 20, got;
    small[k] = malloc(cap);
    while (small[k] && (got = fread(small[k] + small_len[k], 1, cap - small_len[k], f)) > 0)
      if ((small_len[k] += got) == cap) small[k] = realloc(small[k], cap *= 2);
    fclose(f);
    if (!small[k]) return 1;
  }
  pgx_tiling *t = NULL;
  if (pgx_tiling_build(sg, NULL, small[0], small_len[0], small[1], small_len[1], &t)) return fail("graph_to_path.py", "pgx_tiling_build");
  for (int w = 0; w < 2; ++w)
    for (int done = 0; !done;) {
      char *piece = NULL;
      size_t len = 0;
      if (pgx_tiling_text(t, w, (uint64_t)1 << 22, &piece, &len, &done)) return fail("graph_to_path.py", "pgx_tiling_text");
      text[w] = realloc(text[w], text_len[w] + len + 1);
      if (!text[w]) return 1;
      memcpy(text[w] + text_len[w], piece, len), text_len[w] += len;
      pgx_free(piece);
    }
  for (int w = 0; w < 2; ++w) {
    FILE *f = fopen(out_fn[w], "wb");
    if (!f || fwrite(text[w], 1, text_len[w], f) != text_len[w] || fclose(f)) {
      fprintf(stderr, "graph_to_path.py: cannot write %s\n", out_fn[w]);
      return 1;
    }
  }
  for (int w = 0; w < 2; ++w)
    if (fa[w] && pgx_tiling_contigs(t, w, seqdb, fa[w], NULL, NULL)) return fail("graph_to_path.py", "pgx_tiling_contigs");
  pgx_tiling_free(t);
  return 0;
}

int main(int argc, char **argv) {
  char *self = strdup(argv[0]);
  const char *tool = basename(self);
  if (argc > 1 && strcmp(tool, "pgx_cli") == 0) { /* pgx_cli <tool> args... */
    tool = argv[1];
    ++argv, --argc;
  }
  int rc;
  if (strcmp(tool, "shmr_mkseqdb") == 0) rc = main_mkseqdb(argc, argv);
  else if (strcmp(tool, "shmr_index") == 0) rc = main_index(argc, argv);
  else if (strcmp(tool, "shmr_overlap") == 0) rc = main_overlap(argc, argv);
  else if (strcmp(tool, "shmr_dedup") == 0) rc = main_dedup(argc, argv);
  else if (strcmp(tool, "shmr_sgraph") == 0) rc = main_sgraph(argc, argv);
  else if (strcmp(tool, "shmr_map") == 0) rc = main_map(argc, argv);
  else if (strcmp(tool, "path_to_contig.py") == 0) rc = main_path_to_contig(argc, argv);
  else if (strcmp(tool, "graph_to_path.py") == 0) rc = main_graph_to_path(argc, argv);
  else if (strcmp(tool, "pg_asm_cns.py") == 0) rc = main_pg_asm_cns(argc, argv);
  else if (strcmp(tool, "shmr_map_merge") == 0) rc = main_map_merge(argc, argv);
  else if (strcmp(tool, "serve") == 0) rc = main_serve(argc, argv);
  else {
    fprintf(stderr, "usage: pgx_cli {shmr_mkseqdb|shmr_index|shmr_overlap|shmr_dedup|shmr_sgraph|shmr_map|shmr_map_merge|path_to_contig.py|graph_to_path.py|pg_asm_cns.py} [flags]   (or invoke through a link of that name)\n"
                    "       pgx_cli serve -p seqdb_prefix [-i idle_seconds]   (keeps the read database in HBM; the drop-ins attach to it)\n");
    rc = 2;
  }
  fflush(stdout);
  fflush(stderr);
  /* The results are in their files (closed) or on stdout (flushed): leave without tearing the HIP runtime down -- unmapping the
   * device allocations, the pinned pools and the runtime's own threads costs 50-150 ms that no caller waits for anything in.
   * PGX_CLI_TEARDOWN=1 keeps the orderly exit (leak checkers). */
  if (getenv("PGX_CLI_TEARDOWN")) {
    pgx_shutdown();
    free(self);
    return rc;
  }
  _exit(rc);
}
