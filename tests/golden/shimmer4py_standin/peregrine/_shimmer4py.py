"""A stand-in for the reference's cffi module `peregrine._shimmer4py`, for tests/golden/make_golden_contigs.py only: it gives the
reference script py/scripts/path_to_contig.py the `ffi` (new, string, release) and `lib` (ovlp_match, free_ovlp_match, decode_biseq) it
uses, bound with ctypes (cffi is not required) to the REAL reference library compiled in place, oracle/_ref/libshimmer_ref.so.
SHIMMER_REF_LIB names that library; SHIMMER_MATCH_LOG, if set, receives one line `q_m_end t_m_end` per ovlp_match call."""
import ctypes as C
import os
import re

_so = C.CDLL(os.environ["SHIMMER_REF_LIB"])


class _Match(C.Structure):
    _fields_ = [(f, C.c_int32) for f in ("m_size", "dist", "q_bgn", "q_end", "t_bgn", "t_end", "t_m_end", "q_m_end")]


_so.ovlp_match.restype = C.POINTER(_Match)
_so.ovlp_match.argtypes = [C.c_char_p, C.c_int32, C.c_uint8, C.c_char_p, C.c_int32, C.c_uint8, C.c_int32]
_so.free_ovlp_match.argtypes = [C.POINTER(_Match)]
_so.decode_biseq.argtypes = [C.c_char_p, C.c_void_p, C.c_size_t, C.c_uint8]
_log = open(os.environ["SHIMMER_MATCH_LOG"], "w") if os.environ.get("SHIMMER_MATCH_LOG") else None


class _MatchPtr:
    """what cffi hands out for an `ovlp_match_t *`: fields read through the pointer"""

    def __init__(self, p):
        self.p = p

    def __getattr__(self, name):
        return getattr(self.p.contents, name)


class _Lib:
    @staticmethod
    def ovlp_match(q, q_len, q_strand, t, t_len, t_strand, band):
        m = _MatchPtr(_so.ovlp_match(bytes(q), q_len, q_strand, bytes(t), t_len, t_strand, band))
        if _log:
            _log.write(f"{m.q_m_end} {m.t_m_end}\n")
            _log.flush()
        return m

    @staticmethod
    def free_ovlp_match(m):
        _so.free_ovlp_match(m.p)

    @staticmethod
    def decode_biseq(src, seq, length, strand):
        _so.decode_biseq(bytes(src), C.addressof(seq), length, strand)


class _FFI:
    @staticmethod
    def new(decl):
        n = int(re.fullmatch(r"char\[(-?\d+)\]", decl).group(1))
        if n < 0:
            raise ValueError("negative array length")
        return (C.c_char * n)()          # zero-initialised, len() == n, like cffi's char[n]

    @staticmethod
    def string(buf):
        return buf.raw.split(b"\0", 1)[0]   # up to the first NUL or the end of the array

    @staticmethod
    def release(buf):
        pass


ffi, lib = _FFI(), _Lib()
