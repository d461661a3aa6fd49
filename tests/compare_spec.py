"""mnet_compare_stats (include/marconet_hip.h) written out as data: the record of one group in numpy / fp64 over the decoders of tests/storage_codec.py, the
launch arithmetic of marconet_amd/csrc/compare_kernels.hip mirrored, and the case table tests/test_compare_gpu.py runs.  No device use.
tests/test_compare.py proves on a CPU that the spec does what the header says on hand-made cases, that the mirrored constants are the sources', and that
the case table reaches every launch regime of the kernel."""
import numpy as np

from tests import storage_codec as S

# ---- the launch, mirrored (compare_kernels.hip: CMP_THREADS, CMP_UNIT; marconet_hip.h: MNET_CMP_WG_ELEMS, MNET_CMP_MAX_SLICES) ----------------------
THREADS = 256
UNIT = 8                       # elements per thread and trip
WG_ELEMS = THREADS * UNIT      # 2048
MAX_SLICES = 32
RECORD_BYTES = 56

PAIRS = (("f16", "split"), ("mx", "split"), ("f16", "f32"), ("mx", "f32"), ("split", "f32"), ("f32", "f32"))      # (mode, reference) storages
STORAGES = ("f32", "f16", "split", "mx")
DTYPE_ID = {"f32": 0, "f16": 1, "split": 2, "mx": 3}                                                              # mnet_dtype
BYTES_PER_BLOCK = {"f32": 128, "f16": 64, "split": 128, "mx": 128}                                                # per 32 elements
ENCODE = dict(S.ENCODE, f32=lambda v: S.f32(v).view(np.uint8).reshape(S.f32(v).shape[:-1] + (S.f32(v).shape[-1] * 4,)))
DECODE = dict(S.DECODE, f32=lambda raw: np.ascontiguousarray(raw).view(np.uint32))                                # -> fp32 BITS, like S.DECODE


def slices(elems):
    """MNET_CMP_SLICES"""
    return max(1, min(MAX_SLICES, -(-elems // WG_ELEMS)))


def launch(elems):
    """-> (units, slices, trips of slice 0, live threads of the LAST workgroup in its last trip, 0 when that workgroup has no trip of its own)"""
    units = elems // UNIT
    s = slices(elems)
    stride = s * THREADS
    trips0 = -(-units // stride)
    first_last = (s - 1) * THREADS
    trips_last = -(-(units - first_last) // stride) if units > first_last else 0
    live_last = min(THREADS, units - first_last - (trips_last - 1) * stride) if trips_last else 0
    return units, s, trips0, live_last


REGIME = {
    "single_quad": lambda e: launch(e)[0] == 4,
    "sub_wave": lambda e: 4 < launch(e)[0] < 64,
    "ragged_last_workgroup": lambda e: launch(e)[1] > 1 and 0 < launch(e)[3] < THREADS,
    "multi_slice": lambda e: launch(e)[1] > 1,
    "second_trip": lambda e: launch(e)[1] == MAX_SLICES and launch(e)[2] >= 2,
}
# elems_per_group of the GPU cases: the smallest sizes that reach each regime (32: one quad; 96, 224: part of a wave, quads of masked lanes beside live ones;
# 2080: the first size over one workgroup = over one slice, its second workgroup runs one live quad; 4128: three slices; 65568: the first size over the cap —
# workgroup 0 makes a second trip with one live quad, the others none)
SIZES = (32, 96, 224, WG_ELEMS + 32, 2 * WG_ELEMS + 32, MAX_SLICES * WG_ELEMS + 32)
CASE_REGIMES = {32: ("single_quad",), 96: ("sub_wave",), 224: ("sub_wave",), WG_ELEMS + 32: ("multi_slice", "ragged_last_workgroup"),
                2 * WG_ELEMS + 32: ("multi_slice", "ragged_last_workgroup"), MAX_SLICES * WG_ELEMS + 32: ("multi_slice", "second_trip")}
GROUPS = (1, 3)


def plant_positions(elems):
    """element indices at which the maximum is planted: the first and the last element, either side of every slice boundary (and of the boundary between the
    first and the second trip), the first and the last element of the ragged tail's last chunk"""
    units, s, trips0, _ = launch(elems)
    pos = {0, elems - 1, elems - UNIT}
    for k in range(1, s):
        pos |= {k * WG_ELEMS - 1, k * WG_ELEMS}
    if trips0 > 1:
        pos |= {s * WG_ELEMS - 1, s * WG_ELEMS}
    return sorted(p for p in pos if 0 <= p < elems)


# ---- the record ----------------------------------------------------------------------------------------------------------------------------------------
def record(mode_bits, ref_bits):
    """mode_bits, ref_bits: uint32 [elems] — the fp32 BITS the storage's decoder returns.  -> dict, one mnet_cmp_stats"""
    m, r = S.from_bits32(mode_bits).reshape(-1), S.from_bits32(ref_bits).reshape(-1)
    fm, fr = np.isfinite(m), np.isfinite(r)
    both = fm & fr
    out = dict(nonfinite_mode=int((~fm).sum()), nonfinite_ref=int((~fr).sum()))
    if not both.any():
        out.update(max_abs_diff=np.float32(0), max_abs_ref=np.float32(0), max_abs_mode=np.float32(0), argmax_index=-1, sum_sq_diff=0.0, sum_sq_ref=0.0)
        return out
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.abs(np.where(both, m, np.float32(0)) - np.where(both, r, np.float32(0)))          # ONE fp32 subtraction
    d = np.where(both, d, np.float32(-1))
    dmax = d.max()
    out.update(max_abs_diff=np.float32(dmax), argmax_index=int(np.nonzero(d == dmax)[0][0]),
               max_abs_ref=np.float32(np.abs(r[both]).max()), max_abs_mode=np.float32(np.abs(m[both]).max()),
               sum_sq_diff=float((d[both].astype(np.float64) ** 2).sum()), sum_sq_ref=float((r[both].astype(np.float64) ** 2).sum()))
    return out


def records(mode_bits, ref_bits, groups):
    mb, rb = np.asarray(mode_bits).reshape(groups, -1), np.asarray(ref_bits).reshape(groups, -1)
    return [record(mb[g], rb[g]) for g in range(groups)]


RECORD_DTYPE = np.dtype([("max_abs_diff", "<f4"), ("max_abs_ref", "<f4"), ("max_abs_mode", "<f4"), ("reserved", "<i4"), ("argmax_index", "<i8"),
                         ("sum_sq_diff", "<f8"), ("sum_sq_ref", "<f8"), ("nonfinite_mode", "<i8"), ("nonfinite_ref", "<i8")])
assert RECORD_DTYPE.itemsize == RECORD_BYTES
EXACT_FIELDS = ("max_abs_diff", "max_abs_ref", "max_abs_mode", "argmax_index", "nonfinite_mode", "nonfinite_ref")
SUM_FIELDS = ("sum_sq_diff", "sum_sq_ref")
SUM_RTOL = 1e-9               # sizes <= 2^20 elements: n * 2^-53 is below it


def mismatches(got, want):
    """got: RECORD_DTYPE array [groups]; want: list of dicts -> list of strings (empty: equal — maxima, index and counts exactly, sums within SUM_RTOL)"""
    bad = []
    for g, w in enumerate(want):
        for f in EXACT_FIELDS:
            a, b = got[f][g], w[f]
            same = a.tobytes() == np.float32(b).tobytes() if f.startswith("max_") else int(a) == int(b)
            if not same:
                bad.append("group %d %s: got %r, spec %r" % (g, f, a, b))
        for f in SUM_FIELDS:
            a, b = float(got[f][g]), float(w[f])
            if not (abs(a - b) <= SUM_RTOL * abs(b)):
                bad.append("group %d %s: got %r, spec %r" % (g, f, a, b))
        if int(got["reserved"][g]) != 0:
            bad.append("group %d: reserved word %d" % (g, int(got["reserved"][g])))
    return bad


# ---- tensors of the GPU cases ----------------------------------------------------------------------------------------------------------------------------
PLANT = 30000.0               # a half, a split half with lo = 0 and an fp16+8 element with lo8 = 0 alike: every storage holds +-PLANT exactly


def base_values(groups, elems):
    """fp32 [groups, elems]: the finite writer pages of storage_codec back to back (group g starts g pages further on: the groups differ)"""
    flat = S.writer_table().reshape(-1)
    idx = (np.arange(groups)[:, None] * S.PAGE * 3 + np.arange(elems)[None, :]) % flat.size
    return S.f32(flat[idx])


class Operand:
    """one tensor [groups, elems] in a storage: its values, its bytes and what the decoder reads from them, kept in step block by block"""

    def __init__(self, storage, values):
        self.storage, self.v = storage, S.f32(values).copy()
        self.groups, self.elems = self.v.shape
        self.raw = np.ascontiguousarray(ENCODE[storage](self.v.reshape(-1, 32))).reshape(-1, BYTES_PER_BLOCK[storage])      # [blocks, bytes]
        self.bits = np.ascontiguousarray(DECODE[storage](self.raw)).reshape(-1, 32)

    def copy(self):
        o = object.__new__(Operand)
        o.storage, o.groups, o.elems = self.storage, self.groups, self.elems
        o.v, o.raw, o.bits = self.v.copy(), self.raw.copy(), self.bits.copy()
        return o

    def set(self, g, p, value):
        """element p of group g := value (finite); its 32-element block is encoded again"""
        self.v[g, p] = value
        b = (g * self.elems + p) // 32
        blk = self.v.reshape(-1, 32)[b:b + 1]
        self.raw[b] = ENCODE[self.storage](blk).reshape(-1)
        self.bits[b] = DECODE[self.storage](self.raw[b:b + 1]).reshape(-1)

    def poke_nonfinite(self, g, p, value):
        """element p of group g := inf / NaN, written into the stored bytes (the bytes of an fp16+8 block that holds one are not defined by an encoder: the hi
        half is set, which is what makes the element decode non-finite; split half and plain half likewise; fp32: the value itself)"""
        e = g * self.elems + p
        b, c = divmod(e, 32)
        if self.storage == "f32":
            self.raw[b].view(np.float32)[c] = value
        else:
            self.raw[b].view(np.uint16)[c] = np.array([value], dtype=np.float32).astype(np.float16).view(np.uint16)[0]
        self.bits[b] = DECODE[self.storage](self.raw[b:b + 1]).reshape(-1)

    def decoded_bits(self):
        return self.bits.reshape(self.groups, self.elems)
