"""Host-side mirror of the reference interface for the SHIMMER index + overlap path.

`shmr_index(...)` / `shmr_overlap(...)` take the same options as the reference executables
(/root/reference/src/shmr_index.c:64-114, src/shmr_overlap.c:271-326) and produce the same files; the
`ResidentDB` class is the HBM-resident form used by bench.py and the multi-GPU driver.  All compute happens in
libpgx.so on the GPU.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

from . import _lib
from .formats import MC_DTYPE, MM_DTYPE, OVLP_DTYPE, SeqDB


@dataclass
class IndexOut:
    top: np.ndarray            # L1 or L2 minimizers (mm128)
    top_mc: np.ndarray         # (mer, count), sorted by mer
    l0: np.ndarray | None
    l0_mc: np.ndarray | None
    bases: int
    reads: int
    reads_literal: int
    ms: float


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def _take_text(name, call) -> bytes:
    """The text an entry point hands out: call(text, text_len) makes the C call `name` with the two by reference; the bytes are copied
    and the C string goes back (pgx_free)."""
    text, tl = C.c_void_p(), C.c_size_t(0)
    _lib.check(call(C.byref(text), C.byref(tl)), name)
    data = C.string_at(text.value, tl.value)
    _lib.load().pgx_free(text)
    return data


def _text_pieces(fn, name, handle, max_lines):
    """The piece loop of pgx_dedup_drain / pgx_sgraph_text / pgx_unitigs_text: the next lines as bytes of at most max_lines lines each, until
    the call says done.  handle(name) answers the live handle before every call (or raises: the object was closed meanwhile)."""
    done = C.c_int(0)
    while not done.value:
        data = _take_text(name, lambda text, tl: fn(handle(name), int(max_lines), text, tl, C.byref(done)))
        if data:
            yield data


def _rlen_by_rid(rid, rlen) -> np.ndarray:
    """the idx columns as the array the map stage indexes by rid (0 for a rid the idx lacks)"""
    out = np.zeros(int(rid.max()) + 1 if len(rid) else 0, np.uint32)
    out[rid] = rlen
    return out


class ResidentDB:
    """A read database uploaded once to HBM (pgx_seqdb)."""

    def __init__(self, db: SeqDB, device: int | None = None):
        _lib.init(device)
        self._lib = _lib.load()
        self.h = C.c_void_p()
        seq = np.ascontiguousarray(db.seqdb, np.uint8)
        rid = np.ascontiguousarray(db.rid, np.uint32)
        rlen = np.ascontiguousarray(db.rlen, np.uint32)
        roff = np.ascontiguousarray(db.roff, np.uint64)
        _lib.check(self._lib.pgx_seqdb_upload(_ptr(seq), seq.size, _ptr(rid), _ptr(rlen), _ptr(roff), len(rid),
                                              C.byref(self.h)), "pgx_seqdb_upload")
        self.n_reads, self.n_bases = len(rid), int(rlen.sum(dtype=np.uint64))
        self.rlen_by_rid = _rlen_by_rid(rid, rlen)

    @classmethod
    def from_device(cls, d_seqdb: int, nbytes: int, rid, rlen, roff, device: int | None = None):
        """the seqdb bytes are already in HBM at device pointer d_seqdb (e.g. all-gathered by the ranks of a multi-GPU job)"""
        self = cls.__new__(cls)
        _lib.init(device)
        self._lib = _lib.load()
        self.h = C.c_void_p()
        rid = np.ascontiguousarray(rid, np.uint32)
        rlen = np.ascontiguousarray(rlen, np.uint32)
        roff = np.ascontiguousarray(roff, np.uint64)
        _lib.check(self._lib.pgx_seqdb_upload_dev(C.c_void_p(d_seqdb), nbytes, _ptr(rid), _ptr(rlen), _ptr(roff), len(rid),
                                                  C.byref(self.h)), "pgx_seqdb_upload_dev")
        self.n_reads, self.n_bases = len(rid), int(rlen.sum(dtype=np.uint64))
        self.rlen_by_rid = _rlen_by_rid(rid, rlen)
        return self

    @classmethod
    def adopt_device(cls, seq_tensor, nbytes: int, rid, rlen, roff, device: int | None = None):
        """NO copy: the library reads the seqdb where it is -- `seq_tensor` is a torch uint8 device tensor of at least
        nbytes + 1024 elements (e.g. the buffer the ranks of a multi-GPU job all-gathered their read sets into); the object
        keeps it alive.  One copy of the job's seqdb per GPU (pgx_seqdb_adopt_dev)."""
        self = cls.__new__(cls)
        _lib.init(device)
        self._lib = _lib.load()
        self.h = C.c_void_p()
        rid = np.ascontiguousarray(rid, np.uint32)
        rlen = np.ascontiguousarray(rlen, np.uint32)
        roff = np.ascontiguousarray(roff, np.uint64)
        assert seq_tensor.is_contiguous() and seq_tensor.element_size() == 1
        _lib.stream_wait()   # whatever filled the buffer on torch's stream comes first
        _lib.check(self._lib.pgx_seqdb_adopt_dev(C.c_void_p(seq_tensor.data_ptr()), int(nbytes), int(seq_tensor.numel()), _ptr(rid),
                                                 _ptr(rlen), _ptr(roff), len(rid), C.byref(self.h)), "pgx_seqdb_adopt_dev")
        self._adopted = seq_tensor
        self.n_reads, self.n_bases = len(rid), int(rlen.sum(dtype=np.uint64))
        self.rlen_by_rid = _rlen_by_rid(rid, rlen)
        return self

    @classmethod
    def from_fasta(cls, text, device: int | None = None):
        """The database of a FASTA text, made on the GPU (pgx_seqdb_from_fasta): `text` is bytes, or a contiguous torch uint8 device tensor
        (what torch's current stream enqueued comes first).  rid are 0 .. n-1 in text order; `.names` holds the records' names in that
        order; every field and byte is what shmr_mkseqdb and a load of its files give.  FASTQ records, a text without a record and a
        record of 2^32 bases are refused (PgxError)."""
        self = cls.__new__(cls)
        _lib.init(device)
        self._lib = _lib.load()
        self.h = C.c_void_p()
        if isinstance(text, (bytes, bytearray, memoryview)):
            buf = np.frombuffer(text, np.uint8)
            ptr, n, on_dev = _ptr(buf) if len(buf) else None, len(buf), 0
        else:
            assert text.is_cuda and text.is_contiguous() and text.element_size() == 1, "a contiguous uint8 device tensor"
            _lib.stream_wait()
            ptr, n, on_dev = C.c_void_p(text.data_ptr()), int(text.numel()), 1
        names, nl, nr, nb = C.c_void_p(), C.c_size_t(0), C.c_uint64(0), C.c_uint64(0)
        _lib.check(self._lib.pgx_seqdb_from_fasta(ptr, n, on_dev, C.byref(self.h), C.byref(names), C.byref(nl), C.byref(nr), C.byref(nb)),
                   "pgx_seqdb_from_fasta")
        self._names = C.string_at(names.value, nl.value)
        self._lib.pgx_free(names)
        self.names = self._names.decode("latin-1").split("\n")[:-1]
        self.n_reads, self.n_bases = int(nr.value), int(nb.value)
        self.rlen_by_rid = None   # (the lengths stay with the library)
        return self

    @classmethod
    def from_reads(cls, source, device: int | None = None):
        """The database of FASTA/FASTQ reads, made on the GPU (pgx_reads.hip): `source` is the path of a list file as shmr_mkseqdb reads it
        (whitespace-separated paths, plain or .gz: pgx_seqdb_from_files), or a sequence of texts, each one file and each bytes or a
        contiguous torch uint8 device tensor (pgx_seqdb_builder_*).  rid run on across the files; `.names`, `.n_reads`, `.n_bases` and
        `.rlen_by_rid` are set; every field and byte is what shmr_mkseqdb and a load of its files give.  Inputs without a record are
        refused (PgxError)."""
        self = cls.__new__(cls)
        _lib.init(device)
        lib = self._lib = _lib.load()
        self.h = C.c_void_p()
        names, nl, nr, nb = C.c_void_p(), C.c_size_t(0), C.c_uint64(0), C.c_uint64(0)
        if isinstance(source, (str, os.PathLike)):
            _lib.check(lib.pgx_seqdb_from_files(os.fsencode(source), C.byref(self.h), C.byref(names), C.byref(nl), C.byref(nr), C.byref(nb)),
                       "pgx_seqdb_from_files")
        else:
            b = C.c_void_p()
            _lib.check(lib.pgx_seqdb_builder_open(0, C.byref(b)), "pgx_seqdb_builder_open")
            try:
                for text in source:
                    if isinstance(text, (bytes, bytearray, memoryview)):
                        buf = np.frombuffer(text, np.uint8)
                        ptr, n, on_dev = _ptr(buf) if len(buf) else None, len(buf), 0
                    else:
                        assert text.is_cuda and text.is_contiguous() and text.element_size() == 1, "a contiguous uint8 device tensor"
                        _lib.stream_wait()
                        ptr, n, on_dev = C.c_void_p(text.data_ptr()), int(text.numel()), 1
                    _lib.check(lib.pgx_seqdb_builder_feed(b, ptr, n, on_dev, 1), "pgx_seqdb_builder_feed")
                _lib.check(lib.pgx_seqdb_builder_finish(b, C.byref(self.h), C.byref(names), C.byref(nl), C.byref(nr), C.byref(nb)),
                           "pgx_seqdb_builder_finish")
            finally:
                lib.pgx_seqdb_builder_close(b)
        self._names = C.string_at(names.value, nl.value)
        lib.pgx_free(names)
        self.names = self._names.decode("latin-1").split("\n")[:-1]
        self.n_reads, self.n_bases = int(nr.value), int(nb.value)
        self.rlen_by_rid = np.zeros(self.n_reads, np.uint32)
        _lib.check(lib.pgx_seqdb_read_lengths(self.h, _ptr(self.rlen_by_rid), self.n_reads), "pgx_seqdb_read_lengths")
        return self

    def save(self, prefix: str):
        """<prefix>.seqdb and <prefix>.idx of a from_fasta / from_reads database whose bytes are in place (pgx_seqdb_save): shmr_mkseqdb's two files"""
        _lib.check(self._lib.pgx_seqdb_save(self.h, self._names, len(self._names), os.fsencode(prefix)), "pgx_seqdb_save")

    # ---- multi-GPU hand-over on device pointers (include/pgx.h) ------------------------------------------
    def index_dev(self, total_chunk=1, mychunk=1, levels=2, reduction=6, window=80, kmer=16, hpc=False):
        """index stage; returns (IndexOut without arrays, d_top, n_top, d_mc, n_mc): list and counts stay in HBM (library-owned).
        hpc: homopolymer-compressed shimmers (see index)"""
        p = _lib.IndexParams(total_chunk, mychunk, levels, reduction, window, kmer, _lib.want_l0_word(0, hpc))
        r = _lib.IndexResult()
        d_top, n_top, d_mc, n_mc = C.c_void_p(), C.c_size_t(0), C.c_void_p(), C.c_size_t(0)
        _lib.check(self._lib.pgx_index_resident_dev(self.h, C.byref(p), C.byref(r), C.byref(d_top), C.byref(n_top), C.byref(d_mc),
                                                    C.byref(n_mc)), "pgx_index_resident_dev")
        ix = IndexOut(top=None, top_mc=None, l0=None, l0_mc=None, bases=int(r.bases), reads=int(r.reads),
                      reads_literal=int(r.reads_literal), ms=float(r.gpu_ms))
        return ix, int(d_top.value or 0), int(n_top.value), int(d_mc.value or 0), int(n_mc.value)

    def pairs_prepare_dev(self, d_top: int, n_top: int, d_counts_all: int, n_counts_all: int, mc_lower=2, mc_upper=240) -> int:
        first = C.c_int64(-1)
        _lib.check(self._lib.pgx_pairs_prepare_dev(self.h, C.c_void_p(d_top), n_top, C.c_void_p(d_counts_all), n_counts_all,
                                                   mc_lower, mc_upper, C.byref(first)), "pgx_pairs_prepare_dev")
        return int(first.value)

    def pairs_scatter_dev(self, total_chunk: int, start: int):
        """returns (device pointer of the send buffer, records per destination chunk 1..total_chunk)"""
        d_send = C.c_void_p()
        counts = np.zeros(total_chunk, np.uint64)
        _lib.check(self._lib.pgx_pairs_scatter_dev(self.h, total_chunk, start, C.byref(d_send), _ptr(counts)), "pgx_pairs_scatter_dev")
        return int(d_send.value or 0), counts

    def overlap_records_dev(self, d_records: int, n_records: int, total_chunk=1, mychunk=1, bestn=4, mc_lower=2, mc_upper=240,
                            align_bandwidth=100, ovlp_upper=120):
        p = _lib.OverlapParams(total_chunk, mychunk, bestn, mc_lower, mc_upper, align_bandwidth, ovlp_upper)
        out, n, st = C.c_void_p(), C.c_size_t(0), _lib.OverlapStats()
        _lib.check(self._lib.pgx_overlap_records_dev(self.h, C.c_void_p(d_records), n_records, C.byref(p), C.byref(out), C.byref(n),
                                                     C.byref(st)), "pgx_overlap_records_dev")
        return _lib.take(out.value, n.value, OVLP_DTYPE), st.asdict()

    def overlap_dev(self, d_mmers: int, n_mm: int, d_counts: int, n_counts: int, total_chunk=1, mychunk=1, bestn=4, mc_lower=2,
                    mc_upper=240, align_bandwidth=100, ovlp_upper=120):
        p = _lib.OverlapParams(total_chunk, mychunk, bestn, mc_lower, mc_upper, align_bandwidth, ovlp_upper)
        out, n, st = C.c_void_p(), C.c_size_t(0), _lib.OverlapStats()
        _lib.check(self._lib.pgx_overlap_resident_dev(self.h, C.c_void_p(d_mmers), n_mm, C.c_void_p(d_counts), n_counts, C.byref(p),
                                                      C.byref(out), C.byref(n), C.byref(st)), "pgx_overlap_resident_dev")
        return _lib.take(out.value, n.value, OVLP_DTYPE), st.asdict()

    def release_bytes(self) -> bool:
        """The seqdb's BYTES out of HBM (pgx_seqdb_release_bytes): the 2-bit packs carry the same information at a quarter of the size and
        the default path's kernels read them.  Returns False -- bytes kept, nothing changed -- for a database with an ambiguous base or a
        read beyond 65,535 bases; True: an adopted device buffer is no longer referenced (this object drops its hold on it)."""
        rc = self._lib.pgx_seqdb_release_bytes(self.h)
        if rc == _lib.PGX_ESTATE:
            return False
        _lib.check(rc, "pgx_seqdb_release_bytes")
        self._adopted = None
        return True

    def compact_bytes(self) -> bool:
        """release_bytes for a database WITH ambiguous bases (pgx_seqdb_compact_bytes): the bytes of the flagged reads alone stay in HBM (a side
        store), the packs serve everything else, and the byte-wise kernels read those reads' partners from bytes rebuilt out of the packs for
        the call.  Without a flagged read it is release_bytes.  Returns False -- bytes kept, nothing changed -- for a database with a read beyond
        65,535 bases; True: an adopted device buffer is no longer referenced (this object drops its hold on it)."""
        rc = self._lib.pgx_seqdb_compact_bytes(self.h)
        if rc == _lib.PGX_ESTATE:
            return False
        _lib.check(rc, "pgx_seqdb_compact_bytes")
        self._adopted = None
        return True

    @property
    def has_bytes(self) -> bool:
        return bool(self._lib.pgx_seqdb_has_bytes(self.h))

    @property
    def side_bytes(self) -> int:
        """HBM the side store of a compacted database holds (0 before compact_bytes, and without flagged reads)"""
        return int(self._lib.pgx_seqdb_side_bytes(self.h))

    def read_bytes(self, rid: int, length: int) -> np.ndarray:
        """the `length` biseq bytes of read `rid` as the seqdb file holds them (pgx_seqdb_read_bytes): from the bytes, or -- compacted -- from
        the side store / rebuilt from the packs"""
        out = np.zeros(int(length), np.uint8)
        _lib.check(self._lib.pgx_seqdb_read_bytes(self.h, int(rid), _ptr(out), len(out)), "pgx_seqdb_read_bytes")
        return out

    def close(self):
        if self.h:
            self._lib.pgx_seqdb_free(self.h)
            self.h = C.c_void_p()
        self._adopted = None   # (the caller's device buffer is the caller's again)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- stages ------------------------------------------------------------------------------------------
    def index(self, total_chunk=1, mychunk=1, levels=2, reduction=6, window=80, kmer=16, want_l0=False, hpc=False) -> IndexOut:
        """index stage of one chunk.  hpc: homopolymer-compressed shimmers (mm_sketch's is_hpc = 1, minimap2's -H): minimizers of the read with
        every run of equal bases taken as one base, positions and spans in raw coordinates; needs the database's bytes."""
        p = _lib.IndexParams(total_chunk, mychunk, levels, reduction, window, kmer, _lib.want_l0_word(1 if want_l0 else 0, hpc))
        r = _lib.IndexResult()
        _lib.check(self._lib.pgx_index_resident(self.h, C.byref(p), C.byref(r)), "pgx_index_resident")
        return IndexOut(
            top=_lib.take(r.top, r.n_top, MM_DTYPE), top_mc=_lib.take(r.top_mc, r.n_top_mc, MC_DTYPE),
            l0=_lib.take(r.l0, r.n_l0, MM_DTYPE) if want_l0 else None,
            l0_mc=_lib.take(r.l0_mc, r.n_l0_mc, MC_DTYPE) if want_l0 else None,
            bases=int(r.bases), reads=int(r.reads), reads_literal=int(r.reads_literal), ms=float(r.gpu_ms))

    def overlap(self, mmers: np.ndarray, counts: np.ndarray, total_chunk=1, mychunk=1, bestn=4, mc_lower=2,
                mc_upper=240, align_bandwidth=100, ovlp_upper=120):
        mm = np.ascontiguousarray(mmers, MM_DTYPE)
        mc = np.ascontiguousarray(counts, MC_DTYPE)
        p = _lib.OverlapParams(total_chunk, mychunk, bestn, mc_lower, mc_upper, align_bandwidth, ovlp_upper)
        out, n, st = C.c_void_p(), C.c_size_t(0), _lib.OverlapStats()
        _lib.check(self._lib.pgx_overlap_resident(self.h, _ptr(mm), len(mm), _ptr(mc), len(mc), C.byref(p),
                                                  C.byref(out), C.byref(n), C.byref(st)), "pgx_overlap_resident")
        return _lib.take(out.value, n.value, OVLP_DTYPE), st.asdict()

    def index_overlap(self, want_index_arrays=False, levels=2, reduction=6, window=80, kmer=16, bestn=4, mc_lower=2,
                      mc_upper=240, align_bandwidth=100, ovlp_upper=120, hpc=False):
        """single-chunk index + overlap in one call; the shimmer list and its counts never leave HBM between the stages.
        Returns (IndexOut — arrays None unless want_index_arrays —, ovlp records, stats).  hpc: see index."""
        ip = _lib.IndexParams(1, 1, levels, reduction, window, kmer, _lib.want_l0_word(0, hpc))
        op = _lib.OverlapParams(1, 1, bestn, mc_lower, mc_upper, align_bandwidth, ovlp_upper)
        r, out, n, st = _lib.IndexResult(), C.c_void_p(), C.c_size_t(0), _lib.OverlapStats()
        _lib.check(self._lib.pgx_index_overlap_resident(self.h, C.byref(ip), C.byref(op), 1 if want_index_arrays else 0,
                                                        C.byref(r), C.byref(out), C.byref(n), C.byref(st)),
                   "pgx_index_overlap_resident")
        ix = IndexOut(top=_lib.take(r.top, r.n_top, MM_DTYPE) if r.top else None,
                      top_mc=_lib.take(r.top_mc, r.n_top_mc, MC_DTYPE) if r.top_mc else None, l0=None, l0_mc=None,
                      bases=int(r.bases), reads=int(r.reads), reads_literal=int(r.reads_literal), ms=float(r.gpu_ms))
        return ix, _lib.take(out.value, n.value, OVLP_DTYPE), st.asdict()

    # ---- batch level -------------------------------------------------------------------------------------
    def sketch(self, read_slots, w=80, k=16, hpc=False) -> np.ndarray:
        """level-0 minimizers of the listed reads (any 0 < k <= 28, 0 < w < 256); hpc: mm_sketch's is_hpc = 1 (pgx_sketch_batch_hpc)"""
        slots = np.ascontiguousarray(read_slots, np.uint32)
        out, n = C.c_void_p(), C.c_size_t(0)
        name = "pgx_sketch_batch_hpc" if hpc else "pgx_sketch_batch"
        _lib.check(getattr(self._lib, name)(self.h, _ptr(slots), len(slots), w, k, C.byref(out), C.byref(n)), name)
        return _lib.take(out.value, n.value, MM_DTYPE)

    def align(self, keys: np.ndarray, band=100) -> np.ndarray:
        keys = np.ascontiguousarray(keys, _lib.ALIGN_KEY_DTYPE)
        out = np.zeros(len(keys), _lib.MATCH_DTYPE)
        _lib.check(self._lib.pgx_align_batch(self.h, _ptr(keys), len(keys), band, _ptr(out)), "pgx_align_batch")
        return out

    def align2(self, keys: np.ndarray, band=100) -> np.ndarray:
        """align() with a target offset (pgx_align_batch2): the target is read rid1 from byte t_off to its end"""
        keys = np.ascontiguousarray(keys, _lib.ALIGN_KEY2_DTYPE)
        out = np.zeros(len(keys), _lib.MATCH_DTYPE)
        _lib.check(self._lib.pgx_align_batch2(self.h, _ptr(keys), len(keys), band, _ptr(out)), "pgx_align_batch2")
        return out

    def contigs(self, rows: np.ndarray):
        """Contig layout of tiling-path rows (pgx_contigs_resident; _lib.TILE_ROW_DTYPE: contigs numbered 0 .. in order, a contig's rows
        consecutive, s / e as the tiling path gives them).  Returns (bytes, offsets): contig c is bytes[offsets[c]:offsets[c + 1]]."""
        rows = np.ascontiguousarray(rows, _lib.TILE_ROW_DTYPE)
        n_ctg = int(rows["ctg"].max()) + 1 if len(rows) else 0
        off = np.zeros(n_ctg + 1, np.uint64)
        data = _take_text("pgx_contigs_resident",
                          lambda text, tl: self._lib.pgx_contigs_resident(self.h, _ptr(rows), len(rows), n_ctg, text, _ptr(off), tl))
        return data, off


def mm_reduce(mm: np.ndarray, rs: int) -> np.ndarray:
    """GPU mm_reduce over an arbitrary multi-read list (src/shmr_reduce.c:53-90)."""
    _lib.init()
    mm = np.ascontiguousarray(mm, MM_DTYPE)
    out, n = C.c_void_p(), C.c_size_t(0)
    _lib.check(_lib.load().pgx_reduce_batch(_ptr(mm), len(mm), rs, C.byref(out), C.byref(n)), "pgx_reduce_batch")
    return _lib.take(out.value, n.value, MM_DTYPE)


def mm_count(mm: np.ndarray) -> np.ndarray:
    """GPU mm_count (src/shmr_utils.c:131-160); sorted by mer."""
    _lib.init()
    mm = np.ascontiguousarray(mm, MM_DTYPE)
    out, n = C.c_void_p(), C.c_size_t(0)
    _lib.check(_lib.load().pgx_count_batch(_ptr(mm), len(mm), C.byref(out), C.byref(n)), "pgx_count_batch")
    return _lib.take(out.value, n.value, MC_DTYPE)


def _pool_lists(lists):
    """shimmer lists back to back: (the pool, its len(lists) + 1 offsets)"""
    lists = [np.ascontiguousarray(l, MM_DTYPE) for l in lists]
    off = np.zeros(len(lists) + 1, np.uint64)
    np.cumsum([len(l) for l in lists], out=off[1:])
    return (np.concatenate(lists) if lists else np.zeros(0, MM_DTYPE)), off


def shimmer_alns(lists0, lists1, pairs=None, max_diff=100, max_dist=1200, max_repeat=1, direction=0, device=None, stats: dict | None = None):
    """shmr_aln (src/shmr_align.c:21-160) for a batch of list pairs on the GPU (pgx_shmr_aln_batch): the shared shimmers of lists0[a] and
    lists1[b] chained into co-linear runs, chain for chain the reference's.  lists0, lists1: lists of MM_DTYPE arrays; a single array
    for lists0 is that one list against every lists1[j].  pairs: (a, b) index pairs; None pairs lists0[i] with lists1[i].  Returns per
    pair the list of its chains, each an (idx0, idx1) pair of uint32 arrays of equal length, indices into the pair's two lists.
    direction must be 0: the reference's reversed walk reads one entry past its second list and has no answer to reproduce."""
    _lib.init(device)
    one = isinstance(lists0, np.ndarray)
    lists0 = [lists0] if one else list(lists0)
    lists1 = list(lists1)
    if pairs is None:
        if not one and len(lists0) != len(lists1):
            raise ValueError(f"{len(lists0)} lists against {len(lists1)}: give pairs")
        pairs = [(0 if one else i, i) for i in range(len(lists1))]
    pr = np.zeros(len(pairs), _lib.SHMR_ALN_PAIR_DTYPE)
    if len(pairs):
        p = np.asarray(pairs, np.int64).reshape(-1, 2)
        if p.min() < 0 or p.max() >= 2**32:
            raise _lib.PgxError(f"pgx_shmr_aln_batch: a pair names a list out of range ({len(lists0)}, {len(lists1)} lists)")
        pr["list0"], pr["list1"] = p[:, 0], p[:, 1]
    mm0, off0 = _pool_lists(lists0)
    mm1, off1 = _pool_lists(lists1)
    po, co, i0, i1 = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    st = _lib.ShmrAlnStats()
    _lib.check(_lib.load().pgx_shmr_aln_batch(_ptr(mm0), _ptr(off0), len(lists0), _ptr(mm1), _ptr(off1), len(lists1), _ptr(pr), len(pr), int(direction),
                                              int(max_diff), int(max_dist), int(max_repeat), C.byref(po), C.byref(co), C.byref(i0), C.byref(i1), C.byref(st)),
               "pgx_shmr_aln_batch")
    pair_off = _lib.take(po.value, len(pr) + 1, np.dtype("<u8")).astype(np.int64)
    n_chains = int(pair_off[-1])
    chain_off = _lib.take(co.value, n_chains + 1, np.dtype("<u8")).astype(np.int64)
    n_elems = int(chain_off[-1])
    idx0, idx1 = _lib.take(i0.value, n_elems, np.dtype("<u4")), _lib.take(i1.value, n_elems, np.dtype("<u4"))
    if stats is not None:
        stats.update(st.asdict())
    co_l = chain_off.tolist()
    return [[(idx0[co_l[c]:co_l[c + 1]], idx1[co_l[c]:co_l[c + 1]]) for c in range(a, b)] for a, b in zip(pair_off[:-1].tolist(), pair_off[1:].tolist())]


def mmer2tuple(mmer):
    """py/peregrine/utils.py:17-25 on one MM_DTYPE entry: (mmer, span, rid, pos_end, direction)"""
    x, y = int(mmer["x"]), int(mmer["y"])
    return (x >> 8, x & 0xFF, y >> 32, ((y & 0xFFFFFFFF) >> 1) + 1, y & 1)


def get_shimmer_alns(shimmers0, shimmers1, direction=0, max_diff=100, max_dist=1200, max_repeat=1):
    """py/peregrine/utils.py:52-73 on two MM_DTYPE arrays: per chain (the list of (mmer2tuple, mmer2tuple) pairs, np.max(d), np.mean(d),
    np.min(d)).  As in the script, all three numbers come from the LAST pair's d = pos_end0 - pos_end1 alone (it reduces the scalar d,
    not the offsets it collected), so they are equal."""
    shimmers0, shimmers1 = np.ascontiguousarray(shimmers0, MM_DTYPE), np.ascontiguousarray(shimmers1, MM_DTYPE)
    aln_chains = []
    for idx0, idx1 in shimmer_alns(shimmers0, [shimmers1], None, max_diff, max_dist, max_repeat, direction)[0]:
        chain = [(mmer2tuple(shimmers0[a]), mmer2tuple(shimmers1[b])) for a, b in zip(idx0.tolist(), idx1.tolist())]
        d = chain[-1][0][3] - chain[-1][1][3]
        aln_chains.append((chain, np.max(d), np.mean(d), np.min(d)))
    return aln_chains


# ---- file-level stages: drop-ins for the two executables -------------------------------------------------------
def shmr_index(seqdb_prefix: str, out_prefix: str = "shimmer", total_chunk=1, mychunk=1, levels=2, reduction=6,
               write_l0=1, window=80, kmer=16, device=None, hpc=False) -> dict:
    """shmr_index -p -o -t -c -l -r -m -w -k   (defaults of src/shmr_index.c:21-23,49-55), and -H (hpc): homopolymer-compressed shimmers
    under the same file names."""
    _lib.init(device)
    p = _lib.IndexParams(total_chunk, mychunk, levels, reduction, window, kmer, _lib.want_l0_word(write_l0, hpc))
    r = _lib.IndexResult()
    _lib.check(_lib.load().pgx_index_chunk(seqdb_prefix.encode(), out_prefix.encode(), C.byref(p), C.byref(r)),
               "pgx_index_chunk")
    return dict(bases=int(r.bases), reads=int(r.reads), reads_literal=int(r.reads_literal), ms=float(r.gpu_ms))


def shmr_overlap(seqdb_prefix: str, shimmer_prefix: str, out_path: str | None = None, total_chunk=1, mychunk=1,
                 bestn=4, mc_lower=2, mc_upper=240, align_bandwidth=100, ovlp_upper=120, device=None) -> dict:
    """shmr_overlap -p -l -t -c -b -m -M -w -n -o   (defaults of src/shmr_overlap.c:28-42,245-251,341-344)."""
    _lib.init(device)
    if out_path is None:
        out_path = "ovlp.%02d" % mychunk
    p = _lib.OverlapParams(total_chunk, mychunk, bestn, mc_lower, mc_upper, align_bandwidth, ovlp_upper)
    st = _lib.OverlapStats()
    _lib.check(_lib.load().pgx_overlap_chunk(seqdb_prefix.encode(), shimmer_prefix.encode(), out_path.encode(),
                                             C.byref(p), C.byref(st)), "pgx_overlap_chunk")
    return st.asdict()


def shmr_mkseqdb(seq_dataset_path: str = "seq_dataset.lst", seqdb_prefix: str = "seq_dataset", device=None) -> dict:
    """shmr_mkseqdb -d -p   (defaults of src/shmr_mkseqdb.c:61-69): FASTA/FASTQ(.gz) list -> <prefix>.seqdb + <prefix>.idx."""
    _lib.init(device)
    nr, nb = C.c_uint64(0), C.c_uint64(0)
    _lib.check(_lib.load().pgx_mkseqdb(seq_dataset_path.encode(), seqdb_prefix.encode(), C.byref(nr), C.byref(nb)),
               "pgx_mkseqdb")
    return dict(reads=int(nr.value), bases=int(nb.value))


def dedup_piece_records() -> int:
    """records per feed of the file-level dedup (PGX_DEDUP_PIECE, a test hook; default 16 Mi records = 1 GiB)"""
    import os
    return min(max(int(os.environ.get("PGX_DEDUP_PIECE", 0)) or (16 << 20), 1), (1 << 31) - 1)


class DedupStream:
    """shmr_dedup as a stream (pgx_dedup_open / _feed / _close): feed the job's ovlp_t records piece by piece, in bounded memory;
    every feed returns the text lines of the read pairs first seen in it, and the concatenation of the texts is the text of the
    one-shot call on the concatenated records.  expected_pairs sizes the seen-pair set up front (0: it grows as needed).
    graph_ready=True (pgx_dedup_open_graph): every feed returns b"", and after the last one drain() yields only the lines the string
    graph's loader would use -- type `overlap`, two different reads, neither contained by any line of the stream -- in stream order."""

    def __init__(self, expected_pairs: int = 0, device=None, graph_ready: bool = False):
        _lib.init(device)
        self._lib = _lib.load()
        self.h = C.c_void_p()
        self.graph_ready = bool(graph_ready)
        name = "pgx_dedup_open_graph" if graph_ready else "pgx_dedup_open"
        _lib.check(getattr(self._lib, name)(int(expected_pairs), C.byref(self.h)), name)

    def _handle(self, who):
        if not self.h:
            raise _lib.PgxError(f"{who}: the stream is closed")
        return self.h

    def _feed(self, fn, name, ptr, n) -> bytes:
        h = self._handle(name)
        return _take_text(name, lambda text, tl: fn(h, ptr, int(n), text, tl))

    def feed(self, records: np.ndarray) -> bytes:
        """records: ovlp_t records on the host (OVLP_DTYPE)"""
        recs = np.ascontiguousarray(records, OVLP_DTYPE)
        return self._feed(self._lib.pgx_dedup_feed, "pgx_dedup_feed", _ptr(recs), len(recs))

    def feed_dev(self, d_ptr: int, n: int) -> bytes:
        """n ovlp_t records at device pointer d_ptr (e.g. tensor.data_ptr()); what torch's current stream enqueued comes first"""
        import sys
        if "torch" in sys.modules:
            _lib.stream_wait()
        return self._feed(self._lib.pgx_dedup_feed_dev, "pgx_dedup_feed_dev", C.c_void_p(int(d_ptr)), n)

    def drain(self, max_lines: int = 1 << 20):
        """graph_ready streams, after the last feed: the kept lines in order, as bytes of at most max_lines lines each"""
        return _text_pieces(self._lib.pgx_dedup_drain, "pgx_dedup_drain", self._handle, max_lines)

    @property
    def stats(self) -> dict:
        """graph_ready streams: reads marked contained, lines kept (final once drain() has started), lines a plain stream writes"""
        nc, nk, nt = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _lib.check(self._lib.pgx_dedup_graph_stats(self._handle("pgx_dedup_graph_stats"), C.byref(nc), C.byref(nk), C.byref(nt)), "pgx_dedup_graph_stats")
        return dict(contained_reads=int(nc.value), lines_kept=int(nk.value), lines_total=int(nt.value))

    def string_graph(self, min_len: int = 4000, min_idt: float = 96.0, chimer_bridge_removal: bool = False, lfc: bool = False,
                     chimer_ordered: bool = False) -> "StringGraph":
        """graph_ready streams, after the last feed: the string graph of the kept lines (pgx_sgraph_build), what ovlp_to_graph.py's
        generate_string_graph builds with --disable_chimer_bridge_removal and without --lfc.  chimer_ordered runs the script's chimer
        bridge step too, with bfs_nodes' pool popped smallest (rid, end) first (SGRAPH_CHIMER_ORDERED): one of the script's own possible
        answers, and the script's answer wherever it has only one.  chimer_bridge_removal (the step as the script runs it, which has no
        single answer) and lfc are refused, not approximated.  The stream can still be drained or closed; feeds are refused afterwards,
        as after a drain."""
        flags = (SGRAPH_CHIMER_BRIDGE if chimer_bridge_removal else 0) | (SGRAPH_LFC if lfc else 0) | (SGRAPH_CHIMER_ORDERED if chimer_ordered else 0)
        g = C.c_void_p()
        _lib.check(self._lib.pgx_sgraph_build(self._handle("pgx_sgraph_build"), int(min_len), float(min_idt), flags, C.byref(g)), "pgx_sgraph_build")
        return StringGraph(g)

    def close(self):
        """frees the stream; returns (records fed, lines written -- by a plain stream: a graph_ready one reports its kept lines in stats)"""
        nr, nu = C.c_uint64(0), C.c_uint64(0)
        h, self.h = self._handle("pgx_dedup_close"), C.c_void_p()
        _lib.check(self._lib.pgx_dedup_close(h, C.byref(nr), C.byref(nu)), "pgx_dedup_close")
        return int(nr.value), int(nu.value)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if self.h:
            self.close()
        return False

    def __del__(self):
        try:
            if self.h:
                self.close()
        except Exception:
            pass


SGRAPH_CHIMER_BRIDGE, SGRAPH_LFC = 1, 2   # pgx_sgraph_build's flags: both are refused
SGRAPH_CHIMER_ORDERED = 4                 # the chimer bridge step under the stated pop order
SGRAPH_EDGE_DTYPE = np.dtype([("v_rid", "<u4"), ("w_rid", "<u4"), ("label_rid", "<u4"), ("sp", "<i4"), ("tp", "<i4"), ("v_end", "u1"), ("w_end", "u1"),
                              ("type", "u1"), ("pad", "u1"), ("score", "<i8"), ("idt_tenths", "<i8")])   # pgx_sgraph_edge
SGRAPH_TYPES = ("G", "TR", "S", "R", "C")
_SGRAPH_CHIMER_STATS = ("candidates", "past_test1", "chosen", "c_edges")   # pgx_sgraph_chimer_stats_t
_SGRAPH_STATS = ("rows_in", "rows_pass", "edges", "nodes", "n_g", "n_tr", "n_s", "n_r", "max_out_degree", "spur_candidates")


class _DeviceText:
    """A live device object that hands its result out as text: what StringGraph and Unitigs share.  A subclass names its C entry points
    (_STATS_FN, _TEXT_FN, _FREE_FN), the fields of its statistics (_STATS) and how it is spoken of once closed (_CLOSED).
    text(max_lines) yields the lines as bytes of at most max_lines lines each (the next lines: a second iteration goes on where the
    first stopped); write(path) puts the lines not handed out yet into that file (an empty object writes an empty file) and returns the
    bytes written.  close() may be called more than once."""

    def __init__(self, handle):
        self._lib = _lib.load()
        self.h = handle
        st = (C.c_uint64 * len(self._STATS))()
        _lib.check(getattr(self._lib, self._STATS_FN)(self.h, st), self._STATS_FN)
        self.stats = dict(zip(self._STATS, (int(v) for v in st)))

    def _handle(self, who):
        if not self.h:
            raise _lib.PgxError(f"{who}: {self._CLOSED}")
        return self.h

    def text(self, max_lines: int = 1 << 20):
        return _text_pieces(getattr(self._lib, self._TEXT_FN), self._TEXT_FN, self._handle, max_lines)

    def write(self, path: str) -> int:
        n = 0
        with open(path, "wb") as f:
            for piece in self.text():
                f.write(piece)
                n += len(piece)
        return n

    def close(self):
        h, self.h = self.h, C.c_void_p()
        if h:
            _lib.check(getattr(self._lib, self._FREE_FN)(h), self._FREE_FN)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class StringGraph(_DeviceText):
    """The string graph of a graph-mode dedup stream (DedupStream.string_graph): its arrays live on the device and belong to this object,
    whatever becomes of the stream.  Its text is sg_edges_list."""
    _STATS_FN, _TEXT_FN, _FREE_FN = "pgx_sgraph_stats", "pgx_sgraph_text", "pgx_sgraph_free"
    _STATS, _CLOSED = _SGRAPH_STATS, "the graph is closed"

    def edges(self, first: int = 0, n: int | None = None) -> np.ndarray:
        """edge records (SGRAPH_EDGE_DTYPE) in creation order: edge e's reverse is e ^ 1; `type` indexes SGRAPH_TYPES (C only in a graph
        built with chimer_ordered; `stats` counts no C edges)"""
        n = self.stats["edges"] - first if n is None else n
        out = np.zeros(n, SGRAPH_EDGE_DTYPE)
        _lib.check(self._lib.pgx_sgraph_edges(self._handle("pgx_sgraph_edges"), int(first), int(n), _ptr(out)), "pgx_sgraph_edges")
        return out

    @property
    def chimer_stats(self) -> dict:
        """the chimer bridge step's counts (pgx_sgraph_chimer_stats): candidates, of them past test 1, chosen nodes, C edges; zeros for a
        graph built without chimer_ordered"""
        st = (C.c_uint64 * len(_SGRAPH_CHIMER_STATS))()
        _lib.check(self._lib.pgx_sgraph_chimer_stats(self._handle("pgx_sgraph_chimer_stats"), st), "pgx_sgraph_chimer_stats")
        return dict(zip(_SGRAPH_CHIMER_STATS, (int(v) for v in st)))

    def chimers_nodes(self) -> bytes:
        """the chimers_nodes file (pgx_sgraph_chimer_nodes): for every chosen node, in node creation order, its name and then its reverse
        end's, a line each (the script's line order is a set's: compare the sorted lines)"""
        text, n = C.c_void_p(), C.c_size_t(0)
        _lib.check(self._lib.pgx_sgraph_chimer_nodes(self._handle("pgx_sgraph_chimer_nodes"), C.byref(text), C.byref(n)), "pgx_sgraph_chimer_nodes")
        try:
            return C.string_at(text.value, n.value) if n.value else b""
        finally:
            self._lib.pgx_free(text)

    def unitigs(self) -> "Unitigs":
        """the maximal simple paths of the graph's G edges (pgx_sgraph_unitigs); they own their arrays: the graph may be closed first"""
        u = C.c_void_p()
        _lib.check(self._lib.pgx_sgraph_unitigs(self._handle("pgx_sgraph_unitigs"), C.byref(u)), "pgx_sgraph_unitigs")
        return Unitigs(u)

    def tiling(self, utg_text: bytes, ctg_text: bytes) -> "TilingPaths":
        """the tiling paths of this graph's edges, which stay on the device, and the texts of utg_data and ctg_paths (pgx_tiling_build);
        they own their arrays: the graph may be closed first"""
        t = C.c_void_p()
        _lib.check(self._lib.pgx_tiling_build(None, self._handle("pgx_tiling_build"), utg_text, len(utg_text), ctg_text, len(ctg_text), C.byref(t)), "pgx_tiling_build")
        return TilingPaths(t)


def string_graph(records, min_len: int = 4000, min_idt: float = 96.0, device=None, piece: int = 0, chimer_ordered: bool = False) -> StringGraph:
    """The string graph of `records` (OVLP_DTYPE) in one call: a graph-mode dedup stream fed the records (in pieces of `piece`, 0: one
    feed), then DedupStream.string_graph (chimer_ordered: with the chimer bridge step under the stated pop order).  The stream is closed;
    the graph stays."""
    recs = np.ascontiguousarray(records, OVLP_DTYPE)
    piece = piece or max(len(recs), 1)
    with DedupStream(device=device, graph_ready=True) as ds:
        for a in range(0, len(recs), piece):
            ds.feed(recs[a:a + piece])
        return ds.string_graph(min_len, min_idt, chimer_ordered=chimer_ordered)


UNITIG_DTYPE = np.dtype([("s_rid", "<u4"), ("t_rid", "<u4"), ("via_rid", "<u4"), ("s_end", "u1"), ("t_end", "u1"), ("via_end", "u1"), ("circular", "u1"),
                         ("n_edges", "<u4"), ("pad", "<u4"), ("first", "<u8"), ("length", "<i8"), ("score", "<i8")])   # pgx_unitig
_UNITIGS_STATS = ("g_edges", "unitigs", "circular", "longest_edges")   # pgx_unitigs_stats_t


class Unitigs(_DeviceText):
    """The unitigs of a string graph (StringGraph.unitigs, shimmer.unitigs): every maximal simple path of the G edges, numbered by the
    creation index of its first edge.  `via` is always the path's second node and a ring of simple nodes is cut at the tail of its
    smallest-index edge -- the two places where ovlp_to_graph.py's own choice varies with the hash seed.  Their text is the `simple`
    lines of utg_data."""
    _STATS_FN, _TEXT_FN, _FREE_FN = "pgx_unitigs_stats", "pgx_unitigs_text", "pgx_unitigs_free"
    _STATS, _CLOSED = _UNITIGS_STATS, "the unitigs are closed"

    def table(self, first: int = 0, n: int | None = None) -> np.ndarray:
        """UNITIG_DTYPE records: unitig u's edges are paths()[first : first + n_edges]"""
        n = self.stats["unitigs"] - first if n is None else n
        out = np.zeros(n, UNITIG_DTYPE)
        _lib.check(self._lib.pgx_unitigs_table(self._handle("pgx_unitigs_table"), int(first), int(n), _ptr(out)), "pgx_unitigs_table")
        return out

    def paths(self, first: int = 0, n: int | None = None) -> np.ndarray:
        """the creation indices of the G edges, unitig after unitig"""
        n = self.stats["g_edges"] - first if n is None else n
        out = np.zeros(n, np.uint32)
        _lib.check(self._lib.pgx_unitigs_paths(self._handle("pgx_unitigs_paths"), int(first), int(n), _ptr(out)), "pgx_unitigs_paths")
        return out

    def gfa(self, graph_or_edges, db: "ResidentDB | str | None" = None) -> "Gfa":
        """The assembly graph of these unitigs as GFA 1.0 (pgx_gfa_build): graph_or_edges is what they were built from, a live
        StringGraph or the edge records (SGRAPH_EDGE_DTYPE) in creation order; db: the resident reads for the segments' sequences (any
        state), a seqdb prefix (pgx_gfa_build_files: only the reads the segments name are uploaded), or None for the topology-only
        file.  The result owns its arrays."""
        g, e, n = None, None, 0
        if isinstance(graph_or_edges, StringGraph):
            g = graph_or_edges._handle("pgx_gfa_build")
        else:
            e = np.ascontiguousarray(graph_or_edges, SGRAPH_EDGE_DTYPE)
            n = len(e)
            e = e if n else np.zeros(1, SGRAPH_EDGE_DTYPE)       # (no records is still "records": a pointer that is not null)
        f = C.c_void_p()
        if isinstance(db, (str, bytes, os.PathLike)):
            name, src = "pgx_gfa_build_files", os.fsencode(db)
        else:
            name, src = "pgx_gfa_build", db.h if db is not None else None
        _lib.check(getattr(self._lib, name)(self._handle(name), g, None if e is None else _ptr(e), n, src, C.byref(f)), name)
        return Gfa(f)

    def contig_paths(self) -> "ContigPaths":
        """the final utg_data and ctg_paths of these unitigs (pgx_unitigs_contig_paths); utg_text() reads these unitigs' paths: keep them
        open until it was drawn"""
        c = C.c_void_p()
        _lib.check(self._lib.pgx_unitigs_contig_paths(self._handle("pgx_unitigs_contig_paths"), C.byref(c)), "pgx_unitigs_contig_paths")
        return ContigPaths(c, keep=self)


GFA_SEGMENT_DTYPE = np.dtype([("unitig", "<u4"), ("dual", "<u4"), ("n_rows", "<u4"), ("circular", "u1"), ("pad", "u1", (3,)), ("first_row", "<u8"),
                              ("seq_off", "<u8"), ("seq_len", "<u8")])   # pgx_gfa_segment
GFA_LINK_DTYPE = np.dtype([("from_seg", "<u4"), ("to_seg", "<u4"), ("from_rev", "u1"), ("to_rev", "u1"), ("pad", "u1", (2,))])   # pgx_gfa_link
_GFA_STATS = ("unitigs", "segments", "rows", "links_directed", "links", "bases")   # pgx_gfa_stats_t
assert GFA_SEGMENT_DTYPE.itemsize == 40 and GFA_LINK_DTYPE.itemsize == 12


class Gfa:
    """The assembly graph as GFA 1.0 (Unitigs.gfa): every unitig that is smaller than its dual is a segment `utg%06u` of
    its index, with the bases the contig layout makes of its rows when a read database was given; the links join the directed unitigs
    a, b with t(a) == s(b), one of each link and its dual.  stats: the counts; segments() / links() / rows(): the tables
    (GFA_SEGMENT_DTYPE, GFA_LINK_DTYPE, _lib.TILE_ROW_DTYPE); text(): the whole file; write(path): to a file, returns the bytes."""

    def __init__(self, handle):
        self._lib = _lib.load()
        self.h = handle
        st = (C.c_uint64 * len(_GFA_STATS))()
        _lib.check(self._lib.pgx_gfa_stats(self.h, st), "pgx_gfa_stats")
        self.stats = dict(zip(_GFA_STATS, (int(v) for v in st)))

    def _handle(self, who):
        if not self.h:
            raise _lib.PgxError(f"{who}: the GFA is closed")
        return self.h

    def _table(self, name, count, dtype, first, n):
        n = self.stats[count] - first if n is None else n
        out = np.zeros(n, dtype)
        _lib.check(getattr(self._lib, name)(self._handle(name), int(first), int(n), _ptr(out)), name)
        return out

    def segments(self, first: int = 0, n: int | None = None) -> np.ndarray:
        return self._table("pgx_gfa_segments", "segments", GFA_SEGMENT_DTYPE, first, n)

    def links(self, first: int = 0, n: int | None = None) -> np.ndarray:
        return self._table("pgx_gfa_links", "links", GFA_LINK_DTYPE, first, n)

    def rows(self, first: int = 0, n: int | None = None) -> np.ndarray:
        return self._table("pgx_gfa_rows", "rows", _lib.TILE_ROW_DTYPE, first, n)

    def text(self) -> bytes:
        return _take_text("pgx_gfa_text", lambda text, tl: self._lib.pgx_gfa_text(self._handle("pgx_gfa_text"), text, tl))

    def write(self, path: str) -> int:
        _lib.check(self._lib.pgx_gfa_write(self._handle("pgx_gfa_write"), str(path).encode()), "pgx_gfa_write")
        return os.path.getsize(path)

    def close(self):
        h, self.h = self.h, C.c_void_p()
        if h:
            _lib.check(self._lib.pgx_gfa_free(h), "pgx_gfa_free")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


CTG_UNITIG_DTYPE = np.dtype([("type", "<u4"), ("dual", "<u4")])   # pgx_ctg_unitig
CTG_TYPES = ("simple", "spur:2", "simple_dup", "contained", "repeat_bridge", "compound")   # `type` indexes these
CTG_NONE = 0xFFFFFFFF   # the dual of a ring
_CTG_PATHS_STATS = ("unitigs", "simple", "spur2", "simple_dup", "contained", "repeat_bridge", "compound", "ctg_linear", "ctg_circular", "ctg_lines", "row_entries",
                    "longest_ctg", "spur_rounds", "host_us", "device_walks")   # pgx_ctg_paths_stats_t


class ContigPaths:
    """The final unitigs and the contig paths of a string graph (Unitigs.contig_paths, shimmer.contig_paths): what the second half of
    ovlp_to_graph.py writes as utg_data and ctg_paths, by the script's algorithm with every unordered container given an order (DESIGN.md
    4.5e).  stats: the counts; table(): type and dual per unitig (the simple ones as Unitigs numbers them, then the compound ones); rows():
    the unitig indices of every line of ctg_paths; utg_text() / ctg_text(): the two files; tiling(sg): the tiling paths, no file written."""

    def __init__(self, handle, keep=None):
        self._lib = _lib.load()
        self.h = handle
        self._keep = keep   # the unitigs the simple lines are read from, if they are the caller's
        st = (C.c_uint64 * len(_CTG_PATHS_STATS))()
        _lib.check(self._lib.pgx_ctg_paths_stats(self.h, st), "pgx_ctg_paths_stats")
        self.stats = dict(zip(_CTG_PATHS_STATS, (int(v) for v in st)))

    def _handle(self, who):
        if not self.h:
            raise _lib.PgxError(f"{who}: the contig paths are closed")
        return self.h

    def table(self, first: int = 0, n: int | None = None) -> np.ndarray:
        n = self.stats["unitigs"] - first if n is None else n
        out = np.zeros(n, CTG_UNITIG_DTYPE)
        _lib.check(self._lib.pgx_ctg_paths_table(self._handle("pgx_ctg_paths_table"), int(first), int(n), _ptr(out)), "pgx_ctg_paths_table")
        return out

    def rows(self) -> list:
        """per line of ctg_paths its unitigs, as an array of indices"""
        off, u = np.zeros(self.stats["ctg_lines"] + 1, np.uint64), np.zeros(self.stats["row_entries"], np.uint32)
        _lib.check(self._lib.pgx_ctg_paths_rows(self._handle("pgx_ctg_paths_rows"), _ptr(off), _ptr(u)), "pgx_ctg_paths_rows")
        return [u[int(a):int(b)] for a, b in zip(off[:-1], off[1:])]

    def utg_pieces(self, max_lines: int = 1 << 20):
        return _text_pieces(self._lib.pgx_ctg_paths_utg_text, "pgx_ctg_paths_utg_text", self._handle, max_lines)

    def ctg_pieces(self, max_lines: int = 1 << 20):
        return _text_pieces(self._lib.pgx_ctg_paths_ctg_text, "pgx_ctg_paths_ctg_text", self._handle, max_lines)

    def utg_text(self, max_lines: int = 1 << 20) -> bytes:
        """the lines of utg_data not handed out yet"""
        return b"".join(self.utg_pieces(max_lines))

    def ctg_text(self, max_lines: int = 1 << 20) -> bytes:
        """the lines of ctg_paths not handed out yet"""
        return b"".join(self.ctg_pieces(max_lines))

    def write(self, utg_fn: str | None, ctg_fn: str | None) -> int:
        """the two files (None: not that one); returns the bytes written"""
        n = 0
        for fn, pieces in ((utg_fn, self.utg_pieces), (ctg_fn, self.ctg_pieces)):
            if fn is not None:
                with open(fn, "wb") as f:
                    for piece in pieces():
                        f.write(piece)
                        n += len(piece)
        return n

    def tiling(self, sg) -> "TilingPaths":
        """the tiling paths of graph sg (a live StringGraph, or the path of a sg_edges_list file), these unitigs and these contig paths
        (pgx_tiling_build on the two texts; no file is written)"""
        utg, ctg = self.utg_text(), self.ctg_text()
        if isinstance(sg, StringGraph):
            return sg.tiling(utg, ctg)
        t = C.c_void_p()
        _lib.check(self._lib.pgx_tiling_build(str(sg).encode(), None, utg, len(utg), ctg, len(ctg), C.byref(t)), "pgx_tiling_build")
        return TilingPaths(t)

    def close(self):
        h, self.h = self.h, C.c_void_p()
        self._keep = None
        if h:
            _lib.check(self._lib.pgx_ctg_paths_free(h), "pgx_ctg_paths_free")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def contig_paths(edges, device=None) -> ContigPaths:
    """The contig paths of edge records (SGRAPH_EDGE_DTYPE) in creation order, e.g. read_sg_edges_list's, in one call (pgx_ctg_paths_build)"""
    _lib.init(device)
    e = np.ascontiguousarray(edges, SGRAPH_EDGE_DTYPE)
    c = C.c_void_p()
    _lib.check(_lib.load().pgx_ctg_paths_build(_ptr(e) if len(e) else None, len(e), C.byref(c)), "pgx_ctg_paths_build")
    return ContigPaths(c)


def unitigs(edges, device=None) -> Unitigs:
    """The unitigs of edge records (SGRAPH_EDGE_DTYPE) in creation order, e.g. read_sg_edges_list's; only `type` 0 (G) takes part"""
    _lib.init(device)
    e = np.ascontiguousarray(edges, SGRAPH_EDGE_DTYPE)
    u = C.c_void_p()
    _lib.check(_lib.load().pgx_unitigs_build(_ptr(e) if len(e) else None, len(e), C.byref(u)), "pgx_unitigs_build")
    return Unitigs(u)


SGRAPH_TYPE_OTHER = 4   # read_sg_edges_list's `type` of a C edge (the script's chimer bridge step): any value but 0 is "not G"


def read_sg_edges_list(path: str) -> np.ndarray:
    """A sg_edges_list file, whoever wrote it, as edge records (SGRAPH_EDGE_DTYPE) in the file's order: 'v w rid sp tp score identity type'
    with the types G, TR, S, R and C (C becomes SGRAPH_TYPE_OTHER)."""
    code = {b"G": 0, b"TR": 1, b"S": 2, b"R": 3, b"C": SGRAPH_TYPE_OTHER}
    with open(path, "rb") as f:
        lines = f.read().split(b"\n")
    lines = [ln for ln in lines if ln.strip()]
    out = np.zeros(len(lines), SGRAPH_EDGE_DTYPE)
    for k, ln in enumerate(lines):
        f = ln.split()
        if len(f) != 8 or f[7] not in code or f[0][-2:] not in (b":B", b":E") or f[1][-2:] not in (b":B", b":E"):
            raise ValueError(f"{path}: line {k + 1} is not a sg_edges_list line: {ln[:80]!r}")
        t = round(float(f[6]) * 10)
        out[k] = (int(f[0][:-2]) & 0xFFFFFFFF, int(f[1][:-2]) & 0xFFFFFFFF, int(f[2]) & 0xFFFFFFFF, int(f[3]), int(f[4]), f[0][-1:] == b"E", f[1][-1:] == b"E",
                  code[f[7]], 0, int(f[5]), t)
    return out


def parse_sg_edges_list(path: str, hundredths: bool = False):
    """read_sg_edges_list on the device (pgx_sgraph_parse): the file goes up in pieces and a lane tokenises a line.  The same records
    (a type other than G, TR, S, R becomes SGRAPH_TYPE_OTHER; idt_tenths is the exact decimal rounded half to even); with hundredths
    also the identities in hundredths, as an int64 array.  A line that would not print back as it was read is refused (PgxError)."""
    _lib.init(None)
    e, h, n = C.c_void_p(), C.c_void_p(), C.c_uint64(0)
    _lib.check(_lib.load().pgx_sgraph_parse(path.encode(), C.byref(e), C.byref(h), C.byref(n)), "pgx_sgraph_parse")
    edges, hund = _lib.take(e.value, n.value, SGRAPH_EDGE_DTYPE), _lib.take(h.value, n.value, np.dtype("<i8"))
    return (edges, hund) if hundredths else edges


_TILING_STATS = ("sg_lines", "g_edges", "utg_simple", "utg_contained", "utg_compound", "ctg_kept", "ctg_skipped", "ctg_empty", "p_rows", "a_rows", "alternates",
                 "compound_tie_rounds", "host_us")   # pgx_tiling_stats_t
TILING_FILES = ("p_ctg_tiling_path", "a_ctg_tiling_path")   # `which` 0 and 1


class TilingPaths:
    """The tiling paths of a string graph, its unitigs and its contig paths (shimmer.graph_to_path, StringGraph.tiling): what
    graph_to_path.py writes, byte for byte.  `which` is 0 (or "p") for the primary file and 1 (or "a") for the alternate one.
    rows(which): TILE_ROW_DTYPE records, `ctg` indexing names(which); text(which): the lines not handed out yet, as pieces of bytes;
    write(p_path, a_path): both files.  close() may be called more than once."""

    def __init__(self, handle):
        self._lib = _lib.load()
        self.h = handle
        st = (C.c_uint64 * len(_TILING_STATS))()
        _lib.check(self._lib.pgx_tiling_stats(self.h, st), "pgx_tiling_stats")
        self.stats = dict(zip(_TILING_STATS, (int(v) for v in st)))

    def _handle(self, who):
        if not self.h:
            raise _lib.PgxError(f"{who}: the tiling paths are closed")
        return self.h

    @staticmethod
    def _which(which) -> int:
        w = {"p": 0, "a": 1, 0: 0, 1: 1}.get(which)
        if w is None:
            raise ValueError(f"which is 0 / 'p' (primary) or 1 / 'a' (alternate), not {which!r}")
        return w

    def rows(self, which, first: int = 0, n: int | None = None) -> np.ndarray:
        w = self._which(which)
        n = self.stats[("p_rows", "a_rows")[w]] - first if n is None else n
        out = np.zeros(n, _lib.TILE_ROW_DTYPE)
        _lib.check(self._lib.pgx_tiling_rows(self._handle("pgx_tiling_rows"), w, int(first), int(n), _ptr(out)), "pgx_tiling_rows")
        return out

    def names(self, which) -> list:
        w = self._which(which)
        data = _take_text("pgx_tiling_names", lambda text, tl: self._lib.pgx_tiling_names(self._handle("pgx_tiling_names"), w, text, tl, None))
        return data.decode().split("\n")[:-1]

    def text(self, which, max_lines: int = 1 << 20):
        w = self._which(which)
        return _text_pieces(lambda h, ml, text, tl, done: self._lib.pgx_tiling_text(h, w, ml, text, tl, done), "pgx_tiling_text", self._handle, max_lines)

    def write(self, p_path: str, a_path: str) -> int:
        """both files (the lines not handed out yet); the texts are whole in memory before the first file is opened"""
        texts = [b"".join(self.text(w)) for w in (0, 1)]
        for path, data in zip((p_path, a_path), texts):
            with open(path, "wb") as f:
                f.write(data)
        return sum(len(d) for d in texts)

    def contigs(self, which, seqdb_prefix: str, out: str | None = None) -> dict:
        """the contigs of file `which` as FASTA, laid out from the rows on the device (pgx_tiling_contigs): byte for byte what path_to_contig
        makes of the written file, to `out` (None: this process's stdout)"""
        w = self._which(which)
        if out is None:
            import sys
            sys.stdout.flush()
        nc, nb = C.c_uint64(0), C.c_uint64(0)
        _lib.check(self._lib.pgx_tiling_contigs(self._handle("pgx_tiling_contigs"), w, seqdb_prefix.encode(), out.encode() if out is not None else None, C.byref(nc),
                                                C.byref(nb)), "pgx_tiling_contigs")
        return dict(contigs=int(nc.value), bases=int(nb.value))

    def close(self):
        h, self.h = self.h, C.c_void_p()
        if h:
            _lib.check(self._lib.pgx_tiling_free(h), "pgx_tiling_free")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def graph_to_path(sg, utg_data: str, ctg_paths: str, p_out: str | None = None, a_out: str | None = None, device=None, seqdb_prefix: str | None = None,
                  p_ctg_fa: str | None = None, a_ctg_fa: str | None = None):
    """graph_to_path.py: sg is the path of a sg_edges_list file or a live StringGraph; utg_data and ctg_paths are paths.  With p_out and
    a_out the two files are written and the statistics returned (a file path as sg: pgx_tiling_chunk); without, the live TilingPaths.
    p_ctg_fa / a_ctg_fa: also the contigs of that file as FASTA, laid out from the rows with the reads of seqdb_prefix."""
    _lib.init(device)
    if (p_out is None) != (a_out is None):
        raise ValueError("p_out and a_out: both or neither")
    fasta = [(w, fa) for w, fa in ((0, p_ctg_fa), (1, a_ctg_fa)) if fa is not None]
    if fasta and (p_out is None or seqdb_prefix is None):
        raise ValueError("p_ctg_fa / a_ctg_fa need p_out, a_out and seqdb_prefix")
    if isinstance(sg, StringGraph) or p_out is None or fasta:
        with open(utg_data, "rb") as f:
            utg = f.read()
        with open(ctg_paths, "rb") as f:
            ctg = f.read()
        if isinstance(sg, StringGraph):
            t = sg.tiling(utg, ctg)
        else:
            h = C.c_void_p()
            _lib.check(_lib.load().pgx_tiling_build(str(sg).encode(), None, utg, len(utg), ctg, len(ctg), C.byref(h)), "pgx_tiling_build")
            t = TilingPaths(h)
        if p_out is None:
            return t
        with t:
            t.write(p_out, a_out)
            for w, fa in fasta:
                t.contigs(w, seqdb_prefix, fa)
            return t.stats
    st = (C.c_uint64 * len(_TILING_STATS))()
    _lib.check(_lib.load().pgx_tiling_chunk(str(sg).encode(), utg_data.encode(), ctg_paths.encode(), p_out.encode(), a_out.encode(), st), "pgx_tiling_chunk")
    return dict(zip(_TILING_STATS, (int(v) for v in st)))


def shmr_sgraph(ovlp_paths, out_path: str, min_len: int = 4000, min_idt: float = 96.0, device=None, utg_path: str | None = None, utg_data_path: str | None = None,
                ctg_paths_path: str | None = None, chimer_ordered: bool = False, chimers_nodes_path: str | None = None, gfa_path: str | None = None,
                gfa_seqdb: str | None = None) -> dict:
    """cat ovlp*.dat | shmr_sgraph > sg_edges_list: the files through a graph-mode DedupStream piece by piece, the graph, its text to
    out_path (and, with utg_path, its unitigs' lines to that file; with utg_data_path / ctg_paths_path the final utg_data / ctg_paths).
    chimer_ordered: with the chimer bridge step under the stated pop order (DedupStream.string_graph); chimers_nodes_path, valid only with
    it, takes the chimers_nodes file.  gfa_path: the unitig graph as GFA 1.0 to that file (Unitigs.gfa), with the segments' sequences
    from the seqdb prefix gfa_seqdb, topology only without one.  Returns the graph's statistics."""
    if chimers_nodes_path is not None and not chimer_ordered:
        raise ValueError("chimers_nodes_path needs chimer_ordered")
    if gfa_seqdb is not None and gfa_path is None:
        raise ValueError("gfa_seqdb needs gfa_path")
    _lib.init(device)
    if isinstance(ovlp_paths, (str, bytes)):
        ovlp_paths = [ovlp_paths]
    piece = dedup_piece_records()
    with DedupStream(device=device, graph_ready=True) as ds:
        for p in ovlp_paths:
            with open(p, "rb") as f:
                while True:
                    recs = np.fromfile(f, dtype=OVLP_DTYPE, count=piece)
                    if len(recs):
                        ds.feed(recs)
                    if len(recs) < piece:
                        break
        with ds.string_graph(min_len, min_idt, chimer_ordered=chimer_ordered) as g:
            g.write(out_path)
            if chimers_nodes_path is not None:
                with open(chimers_nodes_path, "wb") as f:
                    f.write(g.chimers_nodes())
            if utg_path is not None or utg_data_path is not None or ctg_paths_path is not None or gfa_path is not None:
                with g.unitigs() as u:
                    if gfa_path is not None:
                        with u.gfa(g, gfa_seqdb) as f:
                            f.write(gfa_path)
                    if utg_path is not None:
                        u.write(utg_path)
                    if utg_data_path is not None or ctg_paths_path is not None:
                        with u.contig_paths() as c:
                            c.write(utg_data_path, ctg_paths_path)
            return g.stats


def shmr_dedup(ovlp_paths, out_path: str | None = None, device=None):
    """cat ovlp*.dat | shmr_dedup > preads.ovl (pg_run.py:351-352): returns the text (bytes) and the number of unique pairs.
    The files go through a DedupStream piece by piece; with out_path the text is written as it comes."""
    _lib.init(device)
    if isinstance(ovlp_paths, (str, bytes)):
        ovlp_paths = [ovlp_paths]
    piece = dedup_piece_records()
    parts = []
    out = open(out_path, "wb") if out_path else None
    try:
        with DedupStream(device=device) as ds:
            for p in ovlp_paths:
                with open(p, "rb") as f:
                    while True:
                        recs = np.fromfile(f, dtype=OVLP_DTYPE, count=piece)
                        if len(recs):
                            text = ds.feed(recs)
                            parts.append(text)
                            if out:
                                out.write(text)
                        if len(recs) < piece:
                            break
            _, nu = ds.close()
    finally:
        if out:
            out.close()
    return b"".join(parts), nu


def dedup_graph_ready(records, device=None) -> bytes:
    """shmr_dedup -g in one call: of the text of `records` (OVLP_DTYPE), the lines the string graph's loader would use"""
    with DedupStream(device=device, graph_ready=True) as ds:
        ds.feed(records)
        return b"".join(ds.drain())


def shmr_map(ref_shimmer_prefix: str = "ref-L2", seqdb_prefix: str = "seq_dataset", shimmer_prefix: str = "shimmer-L2",
             refdb_prefix: str = "ref", total_chunk=1, mychunk=1, mc_lower=1, mc_upper=240, out_path: str | None = None, device=None):
    """shmr_map -r -m -p -l -t -c -n -M (src/shmr_map.c:163-373): the reads' shimmer pairs located on the contigs.  Returns the
    reference's stdout text (bytes) and the number of lines."""
    _lib.init(device)
    p = _lib.MapParams(total_chunk, mychunk, mc_lower, mc_upper)
    nl = C.c_uint64(0)
    data = _take_text("pgx_map_chunk", lambda text, tl: _lib.load().pgx_map_chunk(
        refdb_prefix.encode(), ref_shimmer_prefix.encode(), seqdb_prefix.encode(), shimmer_prefix.encode(), C.byref(p), text, tl, C.byref(nl)))
    if out_path:
        with open(out_path, "wb") as f:
            f.write(data)
    return data, int(nl.value)


def path_to_contig(seqdb_prefix: str, tiling_path: str, out: str | None = None, device=None) -> dict:
    """path_to_contig.py seqdb_prefix tiling_path (pgx_contigs_chunk): the contigs of a tiling path as FASTA, byte for byte the script's
    stdout, written to `out` (None: this process's stdout).  Only the reads the path names go to the GPU."""
    _lib.init(device)
    if out is None:
        import sys
        sys.stdout.flush()
    nc, nb = C.c_uint64(0), C.c_uint64(0)
    _lib.check(_lib.load().pgx_contigs_chunk(seqdb_prefix.encode(), tiling_path.encode(), out.encode() if out is not None else None,
                                             C.byref(nc), C.byref(nb)), "pgx_contigs_chunk")
    return dict(contigs=int(nc.value), bases=int(nb.value))


def _cns_rows(pieces):
    """pieces: [(t_len, [(q, t, s1, s2, t_offset), ...]), ...] -> the rows of pgx_cns_aln, both string buffers, the template lengths"""
    n = sum(len(alns) for _, alns in pieces)
    rows = np.zeros(n, _lib.CNS_ALN_DTYPE)
    qs, ts, i, off = [], [], 0, 0
    for p, (_, alns) in enumerate(pieces):
        for q, t, s1, s2, t_offset in alns:
            if len(q) != len(t):
                raise ValueError(f"piece {p}: alignment strings of {len(q)} and {len(t)} bytes")
            rows[i] = (p, t_offset, s1, s2, off, len(q), 0)
            qs.append(bytes(q)); ts.append(bytes(t))
            i, off = i + 1, off + len(q)
    q_str, t_str = np.frombuffer(b"".join(qs), np.uint8), np.frombuffer(b"".join(ts), np.uint8)
    return rows, q_str, t_str, np.array([t_len for t_len, _ in pieces], np.uint32)


def consensus(pieces, min_cov: int = 1, device=None, stats: dict | None = None, on_device: bool = False):
    """get_cns_from_align_tags over get_align_tags (falcon/falcon.c) for a batch of pieces (pgx_cns_call): pieces is a list of
    (template length, [(q_aln_str, t_aln_str, s1, s2, t_offset), ...]) -- what falcon.align answered for every read of the piece, the
    back-bone included -- and the answer one `bytes` per piece, the reference's consensus.  A piece the reference has no answer for raises
    (PGX_EINVAL, the piece named).  stats: filled with pgx_cns_stats.  on_device: upload the inputs with torch and enter through
    pgx_cns_call_dev, as an aligner on the device would."""
    _lib.init(device)
    rows, q_str, t_str, tlen = _cns_rows(pieces)
    off = np.zeros(len(pieces) + 1, np.uint64)
    st = _lib.CnsStats()
    if on_device:
        import torch
        dev = torch.device("cuda", _lib._inited)
        d = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev) for a in (rows, q_str, t_str)]
        torch.cuda.synchronize(dev)
        args, fn, name = [C.c_void_p(x.data_ptr() if x.numel() else 0) for x in d], _lib.load().pgx_cns_call_dev, "pgx_cns_call_dev"
    else:
        args, fn, name = [_ptr(rows), _ptr(q_str), _ptr(t_str)], _lib.load().pgx_cns_call, "pgx_cns_call"
    text = C.c_void_p()
    _lib.check(fn(args[0], len(rows), args[1], args[2], len(q_str), _ptr(tlen), len(pieces), int(min_cov), C.byref(text), _ptr(off), C.byref(st)), name)
    data = C.string_at(text.value, int(off[-1]))
    _lib.load().pgx_free(text)
    if stats is not None:
        stats.update(st.asdict())
    return [data[int(off[p]):int(off[p + 1])] for p in range(len(pieces))]


def align_tags(alns, device=None):
    """get_align_tags (falcon/falcon.c:67-122) for a batch of alignments (pgx_cns_tags): alns is a list of (q_aln_str, t_aln_str, s1, s2,
    t_offset); the answer one array of _lib.CNS_TAG_DTYPE rows per alignment."""
    _lib.init(device)
    rows, q_str, t_str, _ = _cns_rows([(0, list(alns))])
    off = np.zeros(len(rows) + 1, np.uint64)
    tags = C.c_void_p()
    _lib.check(_lib.load().pgx_cns_tags(_ptr(rows), len(rows), _ptr(q_str), _ptr(t_str), len(q_str), C.byref(tags), _ptr(off)), "pgx_cns_tags")
    allt = _lib.take(tags.value, int(off[-1]), _lib.CNS_TAG_DTYPE)
    return [allt[int(off[a]):int(off[a + 1])] for a in range(len(rows))]


def _pool(seqs):
    """byte strings back to back, each stored once (by identity): the pool and where each begins"""
    parts, where, at = [], {}, 0
    for s in seqs:
        if id(s) not in where:
            where[id(s)] = at
            parts.append(bytes(s))
            at += len(s)
    return np.frombuffer(b"".join(parts), np.uint8), where


def falcon_align(pairs, band: int = 150, want_str=True, device=None, stats: dict | None = None):
    """falcon.align (falcon/DW_banded.c) for a batch of pairs (pgx_falcon_align): pairs is a list of (q_bytes, t_bytes) or (q_bytes,
    t_bytes, band); the answer one (aln_str_size, dist, aln_q_s, aln_q_e, aln_t_s, aln_t_e, q_aln_str, t_aln_str) per pair, the fields of the
    reference's `alignment` in its order.  A pair that does not align answers zeros and empty strings.  want_str: one flag for all pairs or
    one per pair; without it the strings are empty and aln_str_size is (q_e + t_e + dist) / 2.  stats: filled with pgx_faln_stats."""
    _lib.init(device)
    pairs = list(pairs)
    want = [bool(want_str)] * len(pairs) if np.ndim(want_str) == 0 else [bool(w) for w in want_str]
    if len(want) != len(pairs):
        raise ValueError(f"{len(want)} want_str flags for {len(pairs)} pairs")
    seq, where = _pool(s for pr in pairs for s in pr[:2])
    reqs = np.zeros(len(pairs), _lib.FALN_REQ_DTYPE)
    for i, pr in enumerate(pairs):
        reqs[i] = (where[id(pr[0])], where[id(pr[1])], len(pr[0]), len(pr[1]), pr[2] if len(pr) > 2 else band, want[i])
    res = np.zeros(len(pairs), _lib.FALN_RES_DTYPE)
    q_str, t_str, nb, st = C.c_void_p(), C.c_void_p(), C.c_uint64(0), _lib.FalnStats()
    _lib.check(_lib.load().pgx_falcon_align(_ptr(reqs), len(reqs), _ptr(seq), len(seq), _ptr(res), C.byref(q_str), C.byref(t_str), C.byref(nb), C.byref(st)),
               "pgx_falcon_align")
    qs, ts = C.string_at(q_str.value, nb.value), C.string_at(t_str.value, nb.value)
    _lib.load().pgx_free(q_str)
    _lib.load().pgx_free(t_str)
    if stats is not None:
        stats.update(st.asdict())
    out = []
    for r, w in zip(res.tolist(), want):
        n = r[0] if w else 0
        out.append((*r[:6], qs[r[6]:r[6] + n], ts[r[6]:r[6] + n]))
    return out


def consensus_reads(pieces, min_cov: int = 1, device=None, stats: dict | None = None, used: list | None = None):
    """pg_asm_cns.py:143-244 for a batch of pieces (pgx_cns_pieces): pieces is a list of (template_bytes, [(read_bytes, read_shift), ...]);
    every read is aligned to its template on the GPU (the back-bone too), kept or dropped by the script's rule, and the pieces answered
    by the consensus call or, where fewer than 3 template lengths aligned, by the template in lower case.  One `bytes` per piece.
    used: a list that receives one bool array per piece (which reads were accepted); stats: filled with pgx_cns_pieces_stats."""
    _lib.init(device)
    pieces = [(t, list(reads)) for t, reads in pieces]
    seq, where = _pool([t for t, _ in pieces] + [r for _, reads in pieces for r, _ in reads])
    pc = np.zeros(len(pieces), _lib.CNS_PIECE_DTYPE)
    rd = np.zeros(sum(len(reads) for _, reads in pieces), _lib.CNS_READ_DTYPE)
    i = 0
    for p, (t, reads) in enumerate(pieces):
        pc[p] = (where[id(t)], len(t), 0)
        for r, shift in reads:
            rd[i] = (where[id(r)], len(r), p, shift, 0)
            i += 1
    off = np.zeros(len(pieces) + 1, np.uint64)
    flags = np.zeros(len(rd), np.uint8)
    text, st = C.c_void_p(), _lib.CnsPiecesStats()
    _lib.check(_lib.load().pgx_cns_pieces(_ptr(pc), len(pc), _ptr(rd), len(rd), _ptr(seq), len(seq), int(min_cov), C.byref(text), _ptr(off), _ptr(flags),
                                          C.byref(st)), "pgx_cns_pieces")
    data = C.string_at(text.value, int(off[-1]))
    _lib.load().pgx_free(text)
    if stats is not None:
        stats.update(st.asdict())
    if used is not None:
        ends = np.cumsum([len(reads) for _, reads in pieces]).tolist()
        used[:] = [flags[e - len(reads):e].astype(bool) for e, (_, reads) in zip(ends, pieces)]
    return [data[int(off[p]):int(off[p + 1])] for p in range(len(pieces))]


def cns_layout(rows, ctg_len, device=None):
    """the layout of pg_asm_cns.py:53-139 (pgx_cns_layout): rows is an (n, 9) integer array of map rows `ctg p1 p2 read rb re strand mc0 mc1`
    that passed the chunk filter, ctg_len the contig lengths by contig id (negative: the idx lacks it).  The answer: (pieces, reads) as
    _lib.CNS_JOB_PIECE_DTYPE and _lib.CNS_JOB_READ_DTYPE arrays, in the order the script answers its segments and aligns their reads."""
    _lib.init(device)
    rows = np.ascontiguousarray(rows, np.int64).reshape(-1, 9)
    lens = np.ascontiguousarray(ctg_len, np.int64)
    pieces, reads, n_piece, n_read = C.c_void_p(), C.c_void_p(), C.c_uint64(0), C.c_uint64(0)
    _lib.check(_lib.load().pgx_cns_layout(_ptr(rows), len(rows), _ptr(lens), len(lens), C.byref(pieces), C.byref(n_piece), C.byref(reads), C.byref(n_read)),
               "pgx_cns_layout")
    return _lib.take(pieces.value, n_piece.value, _lib.CNS_JOB_PIECE_DTYPE), _lib.take(reads.value, n_read.value, _lib.CNS_JOB_READ_DTYPE)


def cns_job_resident(reads: "ResidentDB", ref: "ResidentDB", rows, total_chunks: int, my_chunk: int, ctg_names, stats: dict | None = None):
    """pg_asm_cns.py on two resident databases and all rows of a map (pgx_cns_job_resident): rows is an (n, 9) integer array, ctg_names the
    contigs' names by contig id (a list of str; '' for an id the idx lacks).  The answer: (FASTA bytes, the offsets of the contigs' records
    in it).  stats: filled with pgx_cns_job_stats."""
    rows = np.ascontiguousarray(rows, np.int64).reshape(-1, 9)
    enc = [n.encode() for n in ctg_names]
    name_off = np.concatenate([[0], np.cumsum([len(n) for n in enc])]).astype(np.uint64)
    names = np.frombuffer(b"".join(enc), np.uint8)
    text, off, n_ctg, n_text, st = C.c_void_p(), C.c_void_p(), C.c_uint64(0), C.c_uint64(0), _lib.CnsJobStats()
    _lib.check(_lib.load().pgx_cns_job_resident(reads.h, ref.h, _ptr(rows), len(rows), int(total_chunks), int(my_chunk), _ptr(names), _ptr(name_off), len(enc),
                                                C.byref(text), C.byref(off), C.byref(n_ctg), C.byref(n_text), C.byref(st)), "pgx_cns_job_resident")
    data = C.string_at(text.value, n_text.value)
    offs = np.frombuffer(C.string_at(off.value, 8 * (n_ctg.value + 1)), np.uint64).copy()
    _lib.load().pgx_free(text)
    _lib.load().pgx_free(off)
    if stats is not None:
        stats.update(st.asdict())
    return data, offs


def pg_asm_cns(read_prefix: str, ref_prefix: str, map_path: str, total_chunks: int, my_chunk: int, out: str | None = None, device=None) -> dict:
    """pg_asm_cns.py read_db_prefix ref_db_prefix read_to_contig_map total_chunks my_chunk (pgx_cns_job): the polished contigs of the
    chunk as FASTA, byte for byte the script's stdout, written to `out` (None: this process's stdout).  Returns pgx_cns_job_stats."""
    _lib.init(device)
    if out is None:
        import sys
        sys.stdout.flush()
    st = _lib.CnsJobStats()
    _lib.check(_lib.load().pgx_cns_job(read_prefix.encode(), ref_prefix.encode(), map_path.encode(), int(total_chunks), int(my_chunk),
                                       out.encode() if out is not None else None, C.byref(st)), "pgx_cns_job")
    return st.asdict()


def map_merge(rows_or_paths, out: str | None = None, device=None, stats: dict | None = None):
    """The step between shmr_map and pg_asm_cns.py, `cat map-*.dat | LC_ALL=C sort -k 1 -g -k 2 -g` (pg_run.py:491-496), on the GPU: by
    field 0 and field 1 as numbers, then by the whole line bytewise -- fields 2 .. 8 as decimal strings.
    An (n, 9) integer array of rows (pgx_map_merge_rows): the merged rows come back as an (n, 9) int64 array; `out` is not used.
    A path or a list of paths ("-": stdin) of map chunk files (pgx_map_merge): one merged file is written to `out` (None: this process's
    stdout), and the stats come back.  stats: filled with pgx_map_merge_stats either way."""
    _lib.init(device)
    st = _lib.MapMergeStats()
    if isinstance(rows_or_paths, np.ndarray):
        rows = np.ascontiguousarray(rows_or_paths, np.int64).reshape(-1, 9)
        merged = np.empty_like(rows)
        _lib.check(_lib.load().pgx_map_merge_rows(_ptr(rows), len(rows), _ptr(merged), C.byref(st)), "pgx_map_merge_rows")
        if stats is not None:
            stats.update(st.asdict())
        return merged
    paths = [rows_or_paths] if isinstance(rows_or_paths, (str, bytes, os.PathLike)) else list(rows_or_paths)
    arr = (C.c_char_p * max(len(paths), 1))(*[os.fsencode(p) for p in paths])
    if out is None:
        import sys
        sys.stdout.flush()
    _lib.check(_lib.load().pgx_map_merge(arr, len(paths), os.fsencode(out) if out is not None else None, C.byref(st)), "pgx_map_merge")
    if stats is not None:
        stats.update(st.asdict())
    return st.asdict()


def map_rows(ref_shimmer_prefix: str = "ref-L2", seqdb_prefix: str = "seq_dataset", shimmer_prefix: str = "shimmer-L2", refdb_prefix: str = "ref",
             total_chunk=1, mychunk=1, mc_lower=1, mc_upper=240, device=None) -> np.ndarray:
    """shmr_map answering its rows in place of its text (pgx_map_rows_chunk): an (n, 9) int64 array, a line's nine numbers a row, in the
    order shmr_map prints them -- what map_merge and cns_job_resident take."""
    _lib.init(device)
    p = _lib.MapParams(total_chunk, mychunk, mc_lower, mc_upper)
    rows, n = C.c_void_p(), C.c_uint64(0)
    _lib.check(_lib.load().pgx_map_rows_chunk(refdb_prefix.encode(), ref_shimmer_prefix.encode(), seqdb_prefix.encode(), shimmer_prefix.encode(), C.byref(p),
                                              C.byref(rows), C.byref(n)), "pgx_map_rows_chunk")
    return _lib.take(rows.value, n.value * 9, np.dtype(np.int64)).reshape(-1, 9)


def map_rows_of(ref_mmers, mmers, counts, rlen_by_rid, total_chunk=1, mychunk=1, mc_lower=1, mc_upper=240, device=None) -> np.ndarray:
    """in-memory form of map_rows (pgx_map_rows): arrays in, rows out"""
    _lib.init(device)
    rf = np.ascontiguousarray(ref_mmers, MM_DTYPE)
    mm = np.ascontiguousarray(mmers, MM_DTYPE)
    mc = np.ascontiguousarray(counts, MC_DTYPE)
    rl = np.ascontiguousarray(rlen_by_rid, np.uint32)
    p = _lib.MapParams(total_chunk, mychunk, mc_lower, mc_upper)
    rows, n = C.c_void_p(), C.c_uint64(0)
    _lib.check(_lib.load().pgx_map_rows(_ptr(rf), len(rf), _ptr(mm), len(mm), _ptr(mc), len(mc), _ptr(rl), len(rl), C.byref(p), C.byref(rows), C.byref(n)),
               "pgx_map_rows")
    return _lib.take(rows.value, n.value * 9, np.dtype(np.int64)).reshape(-1, 9)


def consensus_branch(read_prefix: str, read_index_prefix: str, ctg_prefix: str, ctg_index_prefix: str, mapping_nchunk: int, cns_nchunk: int,
                     mc_lower=1, mc_upper=240, out: str | None = None, device=None):
    """The consensus branch of pg_run.py (:389-545) behind the contigs' index, in one process: both databases are loaded once; map_rows for
    the chunks 1 .. mapping_nchunk, map_merge, and cns_job_resident for my = 1 .. cns_nchunk -- the order in which pg_run.py:540-545
    concatenates its chunk files (my == cns_nchunk is chunk 0).  Neither the map text nor the merged file is formed.  The concatenated
    FASTA is returned, or written to `out`."""
    from .formats import read_seqdb
    _lib.init(device)
    read_db, ctg_db = read_seqdb(read_prefix), read_seqdb(ctg_prefix)
    names = [""] * (int(ctg_db.rid.max()) + 1 if ctg_db.n_reads else 0)
    for r, nm in zip(ctg_db.rid, ctg_db.names):
        names[int(r)] = nm
    rdb, cdb = ResidentDB(read_db), ResidentDB(ctg_db)
    try:
        parts = [map_rows(ctg_index_prefix, read_prefix, read_index_prefix, ctg_prefix, mapping_nchunk, c, mc_lower, mc_upper)
                 for c in range(1, int(mapping_nchunk) + 1)]
        rows = map_merge(np.concatenate(parts) if parts else np.zeros((0, 9), np.int64))
        fasta = b"".join(cns_job_resident(rdb, cdb, rows, cns_nchunk, my, names)[0] for my in range(1, int(cns_nchunk) + 1))
    finally:
        rdb.close(), cdb.close()
    if out is not None:
        with open(out, "wb") as f:
            f.write(fasta)
        return len(fasta)
    return fasta


def polish(rdb: "ResidentDB", read_top, read_counts, contig_fasta, mapping_nchunk: int, cns_nchunk: int, levels=2, reduction=6, window=80, kmer=16,
           mc_lower=1, mc_upper=240, out: str | None = None, stats: dict | None = None, hpc=False):
    """The consensus branch of pg_run.py (:401-545) on a read database that is resident already, with its top-level shimmer list and
    counts (all index chunks, concatenated in chunk order), and the contigs as FASTA text (bytes, or a torch uint8 device tensor): the
    contig database straight from the text (ResidentDB.from_fasta), its index with -t 1 -c 1, map_rows_of for the chunks
    1 .. mapping_nchunk, map_merge, cns_job_resident for my = 1 .. cns_nchunk in consensus_branch's order.  No contig file, index file
    or map text is formed.  The concatenated FASTA is returned, or written to `out` (its length returned).
    hpc: the reads' list holds homopolymer-compressed shimmers, so the contigs' index is made of them too."""
    import time
    if rdb.rlen_by_rid is None:
        raise _lib.PgxError("polish: the read database carries no read lengths on the host (a from_fasta database)")
    t = [time.perf_counter()]
    cdb = ResidentDB.from_fasta(contig_fasta)
    try:
        t.append(time.perf_counter())
        ix = cdb.index(1, 1, levels, reduction, window, kmer, hpc=hpc)
        t.append(time.perf_counter())
        parts = [map_rows_of(ix.top, read_top, read_counts, rdb.rlen_by_rid, mapping_nchunk, c, mc_lower, mc_upper) for c in range(1, int(mapping_nchunk) + 1)]
        t.append(time.perf_counter())
        rows = map_merge(np.concatenate(parts) if parts else np.zeros((0, 9), np.int64))
        t.append(time.perf_counter())
        fasta = b"".join(cns_job_resident(rdb, cdb, rows, cns_nchunk, my, cdb.names)[0] for my in range(1, int(cns_nchunk) + 1))
        t.append(time.perf_counter())
        if stats is not None:
            stats.update(contigs=cdb.n_reads, contig_bases=cdb.n_bases, map_rows=len(rows),
                         ms={k: (b - a) * 1e3 for k, a, b in zip(("contig_db", "contig_index", "map", "map_merge", "consensus"), t, t[1:])})
    finally:
        cdb.close()
    if out is not None:
        with open(out, "wb") as f:
            f.write(fasta)
        return len(fasta)
    return fasta


def assemble(seqdb_prefix, index_nchunk: int, ovlp_nchunk: int, mapping_nchunk: int = 0, cns_nchunk: int = 0, min_len: int = 4000,
             min_idt: float = 96.0, with_alt: bool = False, levels=2, reduction=6, window=80, kmer=16, bestn=4, mc_lower=2, mc_upper=240,
             align_bandwidth=100, ovlp_upper=120, chimer_ordered: bool = True, out_dir: str | None = None, device=None, hpc=False,
             gfa: bool = False) -> dict:
    """pg_run.py from the read database on (:227-386 and, with cns_nchunk > 0, :389-565) in one process, on one ResidentDB loaded once:
    every index chunk; every overlap chunk on the concatenated lists and counts; the chunks' records through one graph-mode
    DedupStream in chunk order; the string graph (chimer_ordered: the chimer bridge step, which pg_run.py leaves on, under the stated
    pop order), unitigs, contig paths, tiling paths; the contigs of p (and of a with with_alt) laid out from the rows; polish() on the
    primary FASTA.  mc_lower / mc_upper go to the overlap and to the map stage alike, as pg_run.py passes them.
    seqdb_prefix may be a ResidentDB that carries its read lengths (ResidentDB.from_reads): it is used as it is and left open.
    Returns dict(p_ctg, a_ctg, p_ctg_cns, stats): FASTA bytes (a_ctg / p_ctg_cns None when not asked for) and the stages' statistics
    with their wall times.  With out_dir, p_ctg.fa, a_ctg.fa and p_ctg_cns.fa are written there.  Every handle is closed, also when
    a stage raises.  hpc: every index (reads and contigs) holds homopolymer-compressed shimmers (ResidentDB.index).
    gfa: the result also carries `gfa`, the assembly graph of the phase-1 unitigs with sequences (Unitigs.gfa on the graph and the
    resident reads) as GFA bytes, out_dir gets asm.gfa and stats["ms"] the key "gfa"; without it nothing of that is there."""
    import contextlib
    import time
    from .formats import read_seqdb
    _lib.init(device)
    stats, ms = {}, {}
    clock = [time.perf_counter()]

    def lap(name):
        clock.append(time.perf_counter())
        ms[name] = (clock[-1] - clock[-2]) * 1e3

    def fasta_of(t, which):
        rows, names = t.rows(which), t.names(which)
        if not len(rows):
            return b""
        data, off = rdb.contigs(rows)
        return b"".join(b">" + names[c].encode() + b"\n" + data[int(off[c]):int(off[c + 1])] + b"\n" for c in range(len(off) - 1))

    with contextlib.ExitStack() as es:
        if isinstance(seqdb_prefix, ResidentDB):
            rdb = seqdb_prefix
        else:
            rdb = ResidentDB(read_seqdb(seqdb_prefix), device)
            es.callback(rdb.close)
        lap("load")
        ixs = [rdb.index(index_nchunk, c, levels, reduction, window, kmer, hpc=hpc) for c in range(1, int(index_nchunk) + 1)]
        top = np.concatenate([ix.top for ix in ixs]) if ixs else np.zeros(0, MM_DTYPE)
        counts = np.concatenate([ix.top_mc for ix in ixs]) if ixs else np.zeros(0, MC_DTYPE)
        stats["index"] = [dict(bases=ix.bases, reads=ix.reads, shimmers=len(ix.top)) for ix in ixs]
        lap("index")
        ds = es.enter_context(DedupStream(device=device, graph_ready=True))
        stats["overlap"] = []
        for c in range(1, int(ovlp_nchunk) + 1):
            recs, st = rdb.overlap(top, counts, ovlp_nchunk, c, bestn, mc_lower, mc_upper, align_bandwidth, ovlp_upper)
            ds.feed(recs)
            stats["overlap"].append(st)
        lap("overlap")
        g = es.enter_context(ds.string_graph(min_len, min_idt, chimer_ordered=chimer_ordered))
        stats["dedup"], stats["graph"] = ds.stats, g.stats
        u = es.enter_context(g.unitigs())
        cp = es.enter_context(u.contig_paths())
        t = es.enter_context(cp.tiling(g))
        stats["tiling"] = t.stats
        lap("graph")
        p_ctg = fasta_of(t, 0)
        a_ctg = fasta_of(t, 1) if with_alt else None
        lap("contigs")
        gfa_text = None
        if gfa:
            with u.gfa(g, rdb) as f:
                gfa_text, stats["gfa"] = f.text(), f.stats
            lap("gfa")
        cns = None
        if int(cns_nchunk) > 0:
            stats["polish"] = {}
            cns = b"" if not p_ctg else polish(rdb, top, counts, p_ctg, mapping_nchunk, cns_nchunk, levels, reduction, window, kmer, mc_lower, mc_upper, stats=stats["polish"], hpc=hpc)
            lap("polish")
    stats["ms"] = ms
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        for name, data in (("p_ctg.fa", p_ctg), ("a_ctg.fa", a_ctg), ("p_ctg_cns.fa", cns), ("asm.gfa", gfa_text)):
            if data is not None:
                with open(os.path.join(out_dir, name), "wb") as f:
                    f.write(data)
    out = dict(p_ctg=p_ctg, a_ctg=a_ctg, p_ctg_cns=cns, stats=stats)
    if gfa:
        out["gfa"] = gfa_text
    return out


def map_reads_to_ref(ref_mmers, mmers, counts, rlen_by_rid, total_chunk=1, mychunk=1, mc_lower=1, mc_upper=240, device=None):
    """in-memory form of shmr_map (pgx_map): arrays in, text out"""
    _lib.init(device)
    rf = np.ascontiguousarray(ref_mmers, MM_DTYPE)
    mm = np.ascontiguousarray(mmers, MM_DTYPE)
    mc = np.ascontiguousarray(counts, MC_DTYPE)
    rl = np.ascontiguousarray(rlen_by_rid, np.uint32)
    p = _lib.MapParams(total_chunk, mychunk, mc_lower, mc_upper)
    nl = C.c_uint64(0)
    data = _take_text("pgx_map", lambda text, tl: _lib.load().pgx_map(_ptr(rf), len(rf), _ptr(mm), len(mm), _ptr(mc), len(mc), _ptr(rl), len(rl),
                                                                 C.byref(p), text, tl, C.byref(nl)))
    return data, int(nl.value)


class ShimmerMap:
    """The shimmer4py query object (py_mmer_t + build_shimmer_map4py / get_* of src/shimmer4py.c:44-196), as the reference's
    notebooks and py/peregrine/utils.py use it: built once on the GPU, queried from the host."""

    def __init__(self, seqdb_prefix: str, shimmer_prefix: str, mychunk=1, total_chunk=1, lowerbound=2, upperbound=240, device=None):
        _lib.init(device)
        self._lib = _lib.load()
        self.h = _lib.PyMmer()
        self._lib.build_shimmer_map4py(C.byref(self.h), seqdb_prefix.encode(), shimmer_prefix.encode(), mychunk, total_chunk,
                                       lowerbound, upperbound)
        if not self.h.mmer0_map:
            raise _lib.PgxError("build_shimmer_map4py failed: " + self._lib.pgx_last_error().decode(errors="replace"))

    @property
    def mmers(self) -> np.ndarray:
        v = self.h.mmers.contents
        return np.frombuffer((C.c_uint8 * (v.n * 16)).from_address(v.a), MM_DTYPE) if v.n else np.zeros(0, MM_DTYPE)

    def shimmers_for_read(self, rid: int) -> np.ndarray:
        v = _lib.KVec()
        self._lib.get_shimmers_for_read(C.byref(v), C.byref(self.h), int(rid))
        return np.frombuffer((C.c_uint8 * (v.n * 16)).from_address(v.a), MM_DTYPE).copy() if v.n else np.zeros(0, MM_DTYPE)

    def read_range(self, rid: int):
        """(first index, count) of the read's run inside .mmers"""
        v = _lib.KVec()
        self._lib.get_shimmers_for_read(C.byref(v), C.byref(self.h), int(rid))
        return ((v.a - self.h.mmers.contents.a) // 16 if v.n else 0), int(v.n)

    def mmer_count(self, mhash: int) -> int:
        return int(self._lib.get_mmer_count(C.byref(self.h), int(mhash)))

    def hits(self, mhash0: int, span: int) -> np.ndarray:
        v = _lib.KVec()
        self._lib.get_shimmer_hits(C.byref(v), C.byref(self.h), int(mhash0), int(span))
        out = np.frombuffer(C.string_at(v.a, v.n * _lib.MP256_DTYPE.itemsize), _lib.MP256_DTYPE).copy() if v.n else np.zeros(0, _lib.MP256_DTYPE)
        if v.a:
            self._lib.pgx_free(C.c_void_p(v.a))
        return out

    def close(self):
        if self.h.mmer0_map:
            self._lib.pgx_shimmer_map_free(C.byref(self.h))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
