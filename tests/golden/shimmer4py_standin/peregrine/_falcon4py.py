"""A stand-in for the reference's cffi module `peregrine._falcon4py`, for tests/golden/make_golden_cnsjob.py only: it gives the reference
script py/scripts/pg_asm_cns.py the `ffi` (new, string, release, char-array slicing) and `lib` (align, free_alignment, get_align_tags,
free_align_tags, get_cns_from_align_tags, free_consensus_data) it uses, bound with ctypes (cffi is not required) to the REAL falcon
sources, compiled by the generator into a temporary directory.  FALCON_REF_LIB names that library."""
import ctypes as C
import os
import re

_so = C.CDLL(os.environ["FALCON_REF_LIB"])


class _Alignment(C.Structure):
    _fields_ = [("aln_str_size", C.c_int), ("dist", C.c_int), ("aln_q_s", C.c_int), ("aln_q_e", C.c_int), ("aln_t_s", C.c_int),
                ("aln_t_e", C.c_int), ("q_aln_str", C.c_void_p), ("t_aln_str", C.c_void_p)]


class _AlnRange(C.Structure):
    _fields_ = [("s1", C.c_int), ("e1", C.c_int), ("s2", C.c_int), ("e2", C.c_int), ("score", C.c_long)]


class _AlignTags(C.Structure):
    _fields_ = [("len", C.c_int), ("align_tags", C.c_void_p)]


class _ConsensusData(C.Structure):
    _fields_ = [("sequence", C.c_void_p), ("eqv", C.c_void_p)]


_so.align.restype = C.POINTER(_Alignment)
_so.align.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_int]
_so.free_alignment.argtypes = [C.POINTER(_Alignment)]
_so.get_align_tags.restype = C.POINTER(_AlignTags)
_so.get_align_tags.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(_AlnRange), C.c_uint, C.c_int]
_so.free_align_tags.argtypes = [C.POINTER(_AlignTags)]
_so.get_cns_from_align_tags.restype = C.POINTER(_ConsensusData)
_so.get_cns_from_align_tags.argtypes = [C.POINTER(C.POINTER(_AlignTags)), C.c_uint, C.c_uint, C.c_uint]
_so.free_consensus_data.argtypes = [C.POINTER(_ConsensusData)]


class _Ptr:
    """what cffi hands out for a pointer to a struct: fields read through the pointer"""

    def __init__(self, p):
        self.p = p

    def __getattr__(self, name):
        return getattr(self.p.contents, name)


class _CString:
    """a `char *` field: ffi.string reads up to the NUL"""

    def __init__(self, address):
        self.address = address


class _Cns(_Ptr):
    @property
    def sequence(self):
        return _CString(self.p.contents.sequence)


class _Lib:
    @staticmethod
    def align(q, q_len, t, t_len, band, get_aln_str):
        return _Ptr(_so.align(q, q_len, t, t_len, band, get_aln_str))

    @staticmethod
    def free_alignment(a):
        _so.free_alignment(a.p)

    @staticmethod
    def get_align_tags(q_str, t_str, size, rng, q_id, t_offset):
        return _so.get_align_tags(q_str, t_str, size, rng, q_id, t_offset)

    @staticmethod
    def free_align_tags(tag):
        _so.free_align_tags(tag)

    @staticmethod
    def get_cns_from_align_tags(tags, n, t_len, min_cov):
        return _Cns(_so.get_cns_from_align_tags(tags, n, t_len, min_cov))

    @staticmethod
    def free_consensus_data(c):
        _so.free_consensus_data(c.p)


class _FFI:
    @staticmethod
    def new(decl):
        m = re.fullmatch(r"(char|aln_range|align_tags_t \*) ?\[(-?\d+)\]", decl)
        n = int(m.group(2))
        if n < 0:
            raise ValueError("negative array length")
        kind = {"char": C.c_char, "aln_range": _AlnRange, "align_tags_t *": C.POINTER(_AlignTags)}[m.group(1)]
        return (kind * n)()              # zero-initialised, len() == n, slices of a char array are bytes, like cffi's

    @staticmethod
    def string(buf):
        if isinstance(buf, _CString):
            return C.string_at(buf.address)
        return buf.raw.split(b"\0", 1)[0]   # up to the first NUL or the end of the array

    @staticmethod
    def release(buf):
        pass


ffi, lib = _FFI(), _Lib()
