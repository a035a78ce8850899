"""compress / decompress entry points over the C ABI (include/w3hip.h).

Context wraps one w3_ctx (one GPU).  Host-buffer calls take bytes / numpy
arrays; *_device calls take torch CUDA tensors (PyTorch is only the owner of
device memory and streams here)."""
import ctypes as C

import numpy as np

from . import _lib as L
from .models import HuffCode, Model, W3Error, init_model

MAGIC_STR = b"w30i"  # main.rs:14


def _u8(data):
    if isinstance(data, np.ndarray):
        return np.ascontiguousarray(data, dtype=np.uint8)
    return np.frombuffer(bytes(data), dtype=np.uint8)


def _host_ptr(buf):
    """(address, bytes) of a host buffer: a numpy array, or anything with data_ptr() / numel() / element_size() (a torch CPU tensor —
    pinned ones make the copies asynchronous)."""
    if isinstance(buf, np.ndarray):
        assert buf.flags["C_CONTIGUOUS"]
        return buf.ctypes.data, buf.nbytes
    return buf.data_ptr(), buf.numel() * buf.element_size()


def _ranges(ranges):
    """(ctypes array of w3_range over the numbers, count, sum of the lengths) from a sequence of (offset, len) or an (n, 2) integer array"""
    a = np.asarray(ranges)
    if a.size == 0:
        a = np.zeros((0, 2), dtype=np.uint64)
    if a.dtype.kind not in "iu":
        raise TypeError("ranges must be integers")
    if a.dtype.kind == "i" and (a < 0).any():
        raise ValueError("range offsets and lengths must be non-negative")
    a = np.ascontiguousarray(a.reshape(-1, 2).astype(np.uint64))
    arr = (L.Range * len(a)).from_buffer(a) if len(a) else (L.Range * 1)()   # (the array keeps `a` alive)
    return arr, len(a), int(a[:, 1].sum()) if len(a) else 0


class Context:
    def __init__(self, device=0):
        self.lib = L.load()
        h = C.c_void_p()
        rc = self.lib.w3_ctx_create(device, C.byref(h))
        if rc:
            raise W3Error(rc, "w3_ctx_create(device=%d): no usable HIP device" % device)
        self.h = h
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            self.lib.w3_ctx_destroy(self.h)
            self.h = None

    __del__ = close

    def _chk(self, rc, check=None):
        if rc:
            if rc == L.W3_E_CORRUPT and check is not None:
                raise W3Error(rc, self.lib.w3_last_error(self.h).decode(), bad_block=int(check.bad_block), n_bad=int(check.n_bad))
            raise W3Error(rc, self.lib.w3_last_error(self.h).decode())

    @staticmethod
    def _check(crc):
        """(w3_check over the table, the array that owns it) for a *_checked call"""
        t = np.ascontiguousarray(crc, dtype=np.uint32)
        if t.size == 0:
            t = np.zeros(1, dtype=np.uint32)
        return L.Check(t.ctypes.data, 2**64 - 1, 0), t

    def set_path(self, path):
        self._chk(self.lib.w3_ctx_set_option(self.h, L.W3_OPT_PATH, {"auto": 0, "generic": 1, "twophase": 2}[path]))

    def set_coder(self, mode):
        self._chk(self.lib.w3_ctx_set_option(self.h, L.W3_OPT_CODER, {"x4": 0, "fast": 1, "robust": 2, "x2": 3, "x3": 4, "x5": 5}[mode]))

    def set_acc_limit(self, bits):
        self._chk(self.lib.w3_ctx_set_option(self.h, L.W3_OPT_ACC_LIMIT, bits))

    @staticmethod
    def variant_bits(names):
        """W3_OPT_VARIANT's mask of the names set_variant takes"""
        bits = {"no_lds_atomics": L.W3_VAR_NO_LDS_ATOMICS, "partition4": L.W3_VAR_PARTITION4, "no_chained_partition": L.W3_VAR_NO_CHAINED_PARTITION,
                "cm_unstaged": L.W3_VAR_CM_UNSTAGED, "no_side_stream": L.W3_VAR_NO_SIDE_STREAM, "inject_lds_fault": L.W3_VAR_INJECT_LDS_FAULT,
                "half_cu": L.W3_VAR_HALF_CU, "full_cu": L.W3_VAR_FULL_CU, "slot_table": L.W3_VAR_SLOT_TABLE, "slot_sorted": L.W3_VAR_SLOT_SORTED, "decode_lane": L.W3_VAR_DECODE_LANE,
                "aoh_decode_spec": L.W3_VAR_AOH_DECODE_SPEC, "decode_match_spec": L.W3_VAR_DECODE_MATCH_SPEC}
        v = 0
        for nm in names:
            v |= bits[nm]
        return v

    def set_variant(self, *names):
        """Cross-check hook (W3_OPT_VARIANT): alternative bit-exact implementations, by name: no_lds_atomics, partition4,
        no_chained_partition, cm_unstaged, no_side_stream, half_cu (synchronous calls in the pipeline's kernel shapes), full_cu
        (submitted calls in the plain shapes), slot_table / slot_sorted (slot-state leaves on k_slot / on the sorted replay whatever
        the block count), decode_lane (decode on the lane-per-block kernels, not k_decode_spec / k_aoh_decode_spec), aoh_decode_spec (AC
        over Huffman: the full decode too runs the sixteen-lane decoder where it covers), decode_match_spec (a model with a match-model
        leaf decodes on the sixteen-lane decoder where the rest of it is covered; default: the lane kernels).  No names = defaults."""
        self._chk(self.lib.w3_ctx_set_option(self.h, L.W3_OPT_VARIANT, self.variant_bits(names)))

    def set_verify(self, on=True):
        """W3_OPT_VERIFY: sampled ballot-round re-prediction after every predict phase that used LDS-add rounds (default on)."""
        self._chk(self.lib.w3_ctx_set_option(self.h, L.W3_OPT_VERIFY, int(on)))

    def set_tune(self, bits=0):
        """W3_OPT_TUNE: scheduling experiments of the submit / wait pipeline (set before the first encode_submit)."""
        self._chk(self.lib.w3_ctx_set_option(self.h, L.W3_OPT_TUNE, int(bits)))

    def set_fault_block(self, block=-1):
        """Test hook (with set_variant("inject_lds_fault")): the one block the injected fault hits; -1 = every block."""
        self._chk(self.lib.w3_ctx_set_option(self.h, L.W3_OPT_FAULT_BLOCK, int(block)))

    def set_fault_kernels(self, *names):
        """Test hook (with set_variant("inject_lds_fault")): the kernels whose returning LDS adds the injected fault mis-orders, by
        name: predict_small (the default), rank_sorted, partition8.  No names = the default."""
        bits = {"predict_small": 1, "rank_sorted": 2, "partition8": 4}
        v = 0
        for nm in names:
            v |= bits[nm]
        self._chk(self.lib.w3_ctx_set_option(self.h, L.W3_OPT_FAULT_KERNELS, v or 1))

    def set_slot_budget_mb(self, mb=0):
        self._chk(self.lib.w3_ctx_set_option(self.h, L.W3_OPT_SLOT_BUDGET_MB, int(mb)))

    def set_host_chunk_blocks(self, blocks=0):
        """W3_OPT_HOST_CHUNK_BLOCKS: blocks per pipelined piece of encode_blocks, and per device call of decode_blocks, decode_ranges
        and the aoh_* host-buffer calls (0 = default)."""
        self._chk(self.lib.w3_ctx_set_option(self.h, L.W3_OPT_HOST_CHUNK_BLOCKS, int(blocks)))

    def set_aoh_batch_blocks(self, blocks):
        """W3_OPT_AOH_BATCH_BLOCKS: most blocks per batch of the two-phase form of AC over Huffman, and most jobs per batch of its
        ranges calls and of the sixteen-lane full decode (0 = from the memory budget)."""
        self._chk(self.lib.w3_ctx_set_option(self.h, L.W3_OPT_AOH_BATCH_BLOCKS, int(blocks)))

    def set_export_epoch(self, nbytes=0):
        """W3_OPT_EXPORT_EPOCH: bytes per epoch of export_counters_device / export_counters_staged (0 = default; a multiple of 1 KiB, at
        most 2^28; the result is the same)."""
        self._chk(self.lib.w3_ctx_set_option(self.h, L.W3_OPT_EXPORT_EPOCH, int(nbytes)))

    def set_wave_grid(self, n=0):
        """W3_OPT_WAVE_GRID: most wavefronts the predict phase's k_match_keys and k_predict_wave launches take, so that one wavefront
        walks several blocks over its private table (0 = default; the output is the same).  What a call ran with: last_wave_grid()."""
        self._chk(self.lib.w3_ctx_set_option(self.h, L.W3_OPT_WAVE_GRID, int(n)))

    def last_wave_grid(self):
        """w3_last_wave_grid: (k_match_keys grid, k_predict_wave grid) of this context's most recent two-phase predict phase; 0 where
        that kernel was not launched, the smallest of several k_predict_wave leaves'"""
        out = (C.c_uint32 * 2)()
        self._chk(self.lib.w3_last_wave_grid(self.h, C.byref(out)))
        return int(out[0]), int(out[1])

    def set_timing(self, on=True):
        self._chk(self.lib.w3_ctx_set_option(self.h, L.W3_OPT_TIMING, int(on)))

    def timing(self):
        t = L.Timing()
        self._chk(self.lib.w3_get_timing(self.h, C.byref(t)))
        return {k: (list(getattr(t, k)) if k in ("part_ms", "rank_ms") else getattr(t, k)) for k, _ in L.Timing._fields_}

    # ---- host buffers ----------------------------------------------------
    def encode_blocks(self, model, data, block_size, out_cap=None):
        """-> (concatenated streams: np.uint8[], block_lens: np.uint32[])"""
        spec = model.spec() if isinstance(model, Model) else model
        a = _u8(data)
        n = len(a)
        nb = (n + block_size - 1) // block_size if block_size else 0
        if out_cap is None:
            out_cap = 2 * n + 64 * nb + 64
        while True:
            out = np.empty(max(out_cap, 1), dtype=np.uint8)
            lens = np.zeros(max(nb, 1), dtype=np.uint32)
            olen = C.c_size_t()
            rc = self.lib.w3_encode_blocks(self.h, C.byref(spec), a.ctypes.data_as(C.c_void_p), n, block_size,
                                           out.ctypes.data_as(C.c_void_p), out_cap, C.byref(olen), lens.ctypes.data_as(C.c_void_p))
            if rc == L.W3_E_NOSPACE and olen.value > out_cap:
                out_cap = olen.value
                continue
            self._chk(rc)
            return out[: olen.value], lens[:nb]

    def encode_host_submit(self, model, data, block_size, out, lens):
        """w3_encode_host_submit: `data`, `out` (uint8) and `lens` (uint32[nb]) are host buffers — numpy arrays or torch CPU tensors,
        pinned or not — that must stay alive and untouched until encode_host_wait(job).  -> job handle"""
        spec = model.spec() if isinstance(model, Model) else model
        ip, n = _host_ptr(data)
        op, cap = _host_ptr(out)
        lp, _ = _host_ptr(lens)
        job = C.c_int(-1)
        self._chk(self.lib.w3_encode_host_submit(self.h, C.byref(spec), C.c_void_p(ip), n, block_size, C.c_void_p(op), cap, C.c_void_p(lp), C.byref(job)))
        return job.value

    def encode_host_wait(self, job):
        """w3_encode_host_wait -> compressed bytes now in the job's `out` (raises what w3_encode_blocks would have raised)."""
        olen = C.c_size_t()
        rc = self.lib.w3_encode_host_wait(self.h, int(job), C.byref(olen))
        self._chk(rc)
        return olen.value

    def host_max_in_flight(self, n, block_size, model=None):
        spec = None if model is None else (model.spec() if isinstance(model, Model) else model)
        return int(self.lib.w3_encode_host_max_in_flight(C.byref(spec) if spec is not None else None, int(n), int(block_size)))

    def decode_blocks(self, model, comp, block_lens, block_size, orig_len, crc=None):
        """crc: the CRC-32 table of the original blocks (crc32_blocks) — w3_decode_blocks_checked: every decoded block is verified on the
        device, W3Error(W3_E_CORRUPT) with .bad_block and .n_bad when one differs.  None: w3_decode_blocks."""
        spec = model.spec() if isinstance(model, Model) else model
        a = _u8(comp)
        lens = np.ascontiguousarray(block_lens, dtype=np.uint32)
        out = np.empty(max(orig_len, 1), dtype=np.uint8)
        args = (self.h, C.byref(spec), a.ctypes.data_as(C.c_void_p), len(a), lens.ctypes.data_as(C.c_void_p),
                len(lens), block_size, orig_len, out.ctypes.data_as(C.c_void_p))
        if crc is None:
            self._chk(self.lib.w3_decode_blocks(*args))
        else:
            ck, _keep = self._check(crc)
            self._chk(self.lib.w3_decode_blocks_checked(*args, C.byref(ck)), ck)
        return out[:orig_len]

    # ---- CRC-32 per block (include/w3hip.h "integrity") ----
    def crc32_blocks(self, data, block_size):
        """w3_crc32_blocks: zlib's CRC-32 of every block of `data`, computed on the device.  -> np.uint32[nblocks]"""
        a = _u8(data)
        nb = (len(a) + block_size - 1) // block_size if block_size else 0
        crc = np.zeros(max(nb, 1), dtype=np.uint32)
        self._chk(self.lib.w3_crc32_blocks(self.h, a.ctypes.data_as(C.c_void_p), len(a), block_size, crc.ctypes.data_as(C.c_void_p)))
        return crc[:nb]

    def crc32_blocks_device(self, d_in, block_size, d_crc, stream=None):
        """w3_crc32_blocks_device: d_in torch.uint8 CUDA tensor, d_crc int32/uint32[nblocks] CUDA tensor receiving the table."""
        st = C.c_void_p(stream) if stream else None
        self._chk(self.lib.w3_crc32_blocks_device(self.h, C.c_void_p(d_in.data_ptr()), d_in.numel(), block_size, C.c_void_p(d_crc.data_ptr()), st))

    # ---- table preparation on the device (include/w3hip.h; csrc/w3_prep.h) ----
    def histogram(self, data):
        """w3_histogram: the byte histogram of host `data` of any length, counted on the device.  -> np.uint64[256]"""
        a = _u8(data)
        counts = np.zeros(256, dtype=np.uint64)
        self._chk(self.lib.w3_histogram(self.h, a.ctypes.data_as(C.c_void_p), len(a), counts.ctypes.data_as(C.c_void_p)))
        return counts

    def histogram_device(self, d_in, stream=None):
        """w3_histogram_device: d_in a torch.uint8 CUDA tensor (contiguous).  -> np.uint64[256] on the host"""
        st = C.c_void_p(stream) if stream else None
        counts = np.zeros(256, dtype=np.uint64)
        self._chk(self.lib.w3_histogram_device(self.h, C.c_void_p(d_in.data_ptr()), d_in.numel(), counts.ctypes.data_as(C.c_void_p), st))
        return counts

    def histogram_of(self, data):
        """histogram_device for a tensor (anything with data_ptr()), histogram for host data"""
        return self.histogram_device(data) if hasattr(data, "data_ptr") else self.histogram(data)

    def stationary_table(self, data, stream=None):
        """StationaryModel::new's table on the device: w3_stationary_table_device for a torch.uint8 CUDA tensor, w3_stationary_table_staged
        for host data of any length.  -> list of 8 ints"""
        t = (C.c_uint16 * 8)()
        if hasattr(data, "data_ptr"):
            st = C.c_void_p(stream) if stream else None
            self._chk(self.lib.w3_stationary_table_device(self.h, C.c_void_p(data.data_ptr()), data.numel(), t, st))
        else:
            a = _u8(data)
            self._chk(self.lib.w3_stationary_table_staged(self.h, a.ctypes.data_as(C.c_void_p), len(a), t))
        return list(t)

    def table_prep_profile(self, d_in, hist_rep=L.W3_HIST_REP):
        """w3_table_prep_profile (tools/table_prep_rate.py): both preparations of the tensor d_in once, each kernel's time from HIP events"""
        p = L.PrepProfile()
        self._chk(self.lib.w3_table_prep_profile(self.h, C.c_void_p(d_in.data_ptr()), d_in.numel(), int(hist_rep), C.byref(p)))
        return {"hist_ms": p.hist_ms, "hist_sum_ms": p.hist_sum_ms, "stat_count_ms": p.stat_count_ms, "stat_walk_ms": p.stat_walk_ms,
                "halvings": list(p.halvings), "table": list(p.table), "counts": np.array(p.counts, dtype=np.uint64)}

    def crc32_verify_device(self, d_data, block_size, d_crc, stream=None):
        """w3_crc32_verify_device: the blocks of d_data against the table d_crc (both CUDA tensors).  -> (bad_block, n_bad) = (2**64 - 1, 0)
        when every block matches; W3Error(W3_E_CORRUPT) with .bad_block (the lowest block that differs) and .n_bad otherwise."""
        st = C.c_void_p(stream) if stream else None
        bad, nbad = C.c_uint64(2**64 - 1), C.c_uint64(0)
        rc = self.lib.w3_crc32_verify_device(self.h, C.c_void_p(d_data.data_ptr()), d_data.numel(), block_size, C.c_void_p(d_crc.data_ptr()),
                                             C.byref(bad), C.byref(nbad), st)
        if rc == L.W3_E_CORRUPT:
            raise W3Error(rc, self.lib.w3_last_error(self.h).decode(), bad_block=bad.value, n_bad=nbad.value)
        self._chk(rc)
        return bad.value, nbad.value

    def decode_ranges(self, model, comp, block_lens, block_size, orig_len, ranges, crc=None):
        """Random access (w3_decode_ranges): the bytes of `ranges` — (offset, len) pairs or an (n, 2) integer array — of the original data,
        concatenated in request order, decoding only the blocks they touch.  -> np.uint8[sum of the lengths]
        crc: the CRC-32 table of ALL the container's blocks — w3_decode_ranges_checked: every touched block is decoded whole and verified."""
        spec = model.spec() if isinstance(model, Model) else model
        a = _u8(comp)
        lens = np.ascontiguousarray(block_lens, dtype=np.uint32)
        rs, n, total = _ranges(ranges)
        out = np.empty(max(total, 1), dtype=np.uint8)
        olen = C.c_size_t()
        args = (self.h, C.byref(spec), a.ctypes.data_as(C.c_void_p), len(a), lens.ctypes.data_as(C.c_void_p), len(lens),
                block_size, orig_len, rs, n, out.ctypes.data_as(C.c_void_p), total, C.byref(olen))
        if crc is None:
            self._chk(self.lib.w3_decode_ranges(*args))
        else:
            ck, _keep = self._check(crc)
            self._chk(self.lib.w3_decode_ranges_checked(*args, C.byref(ck)), ck)
        return out[: olen.value]

    def encode_stats(self, model, data, block_size):
        """ACStats (helpers.rs:60-90) per block: the bit counts the reference's `csize = bits / 8` comes from.  -> np.uint32[nb]"""
        spec = model.spec() if isinstance(model, Model) else model
        a = _u8(data)
        nb = (len(a) + block_size - 1) // block_size if block_size else 0
        bits = np.zeros(max(nb, 1), dtype=np.uint32)
        self._chk(self.lib.w3_encode_stats(self.h, C.byref(spec), a.ctypes.data_as(C.c_void_p), len(a), block_size, bits.ctypes.data_as(C.c_void_p)))
        return bits[:nb]

    def sweep_ordern(self, data, block_size, configs):
        """OrderN(bits, align) for every (bits, align) in `configs`, all in one device launch (bin/ordern/main.rs:9-80).
        -> np.uint32[len(configs)][nb] ACStats bit counts."""
        a = _u8(data)
        nb = (len(a) + block_size - 1) // block_size if block_size else 0
        cb = np.array([c[0] for c in configs], dtype=np.uint8)
        ca = np.array([c[1] for c in configs], dtype=np.uint8)
        out = np.zeros((len(configs), max(nb, 1)), dtype=np.uint32)
        self._chk(self.lib.w3_sweep_ordern(self.h, a.ctypes.data_as(C.c_void_p), len(a), block_size, cb.ctypes.data_as(C.c_void_p),
                                           ca.ctypes.data_as(C.c_void_p), len(configs), out.ctypes.data_as(C.c_void_p)))
        return out[:, :nb]

    def export_counters(self, model, data):
        """Context statistics export (README.md:9): the model's Counter table after `data` as one stream.
        -> (n0: np.uint16[2^bits], n1: np.uint16[2^bits])"""
        spec = model.spec()
        a = _u8(data)
        bits = spec.nodes[0].bits
        t = np.zeros(1 << bits, dtype=np.uint32)
        self._chk(self.lib.w3_export_counters(self.h, C.byref(spec), a.ctypes.data_as(C.c_void_p), len(a), t.ctypes.data_as(C.c_void_p)))
        return (t & 0xFFFF).astype(np.uint16), (t >> 16).astype(np.uint16)

    def _export_device(self, fn, model, d_in, d_counters, stream):
        """the device form of both exports: fn = the library's w3_export_counters_device or w3_export_entropy_device"""
        import torch
        if d_in.dtype != torch.uint8 or not d_in.is_cuda or not d_in.is_contiguous():
            raise W3Error(L.W3_E_INVALID, "d_in: a contiguous torch.uint8 CUDA tensor")
        spec = model.spec()
        entries = 1 << spec.nodes[0].bits
        if d_counters is None:
            if spec.n_nodes != 1 or spec.nodes[0].bits > 28:   # (refused below, before the tensor is touched: do not allocate 2^bits for it)
                entries = 1
            d_counters = torch.empty(entries, dtype=torch.int32, device=d_in.device)
        elif (d_counters.dtype != torch.int32 or d_counters.numel() != entries or not d_counters.is_contiguous()
              or d_counters.device != d_in.device):
            raise W3Error(L.W3_E_INVALID, "d_counters: a contiguous torch.int32 tensor of 2^bits entries on d_in's device")
        st = C.c_void_p(stream) if stream else None
        self._chk(fn(self.h, C.byref(spec), C.c_void_p(d_in.data_ptr()), d_in.numel(), C.c_void_p(d_counters.data_ptr()), st))
        return d_counters

    def _export_staged(self, fn, model, data):
        """the staged form of both exports: fn = the library's w3_export_counters_staged or w3_export_entropy_staged"""
        spec = model.spec()
        a = _u8(data)
        refused = spec.n_nodes != 1 or spec.nodes[0].bits > 28
        t = np.zeros(1 if refused else 1 << spec.nodes[0].bits, dtype=np.uint32)
        self._chk(fn(self.h, C.byref(spec), a.ctypes.data_as(C.c_void_p), len(a), t.ctypes.data_as(C.c_void_p)))
        return (t & 0xFFFF).astype(np.uint16), (t >> 16).astype(np.uint16)

    def export_counters_device(self, model, d_in, d_counters=None, stream=None):
        """w3_export_counters_device: the same table for ONE adaptive OrderN leaf without entropy history, computed in parallel over the
        whole input (csrc/w3_export.h).  d_in: a torch.uint8 CUDA tensor (contiguous).  -> a torch.int32 CUDA tensor of 2^bits packed
        counters n0 | n1 << 16 (d_counters when given: every entry is overwritten)"""
        return self._export_device(self.lib.w3_export_counters_device, model, d_in, d_counters, stream)

    def export_counters_staged(self, model, data):
        """w3_export_counters_staged: the same from host `data` of any length, staged through the device in pieces.
        -> (n0: np.uint16[2^bits], n1: np.uint16[2^bits]), the shape export_counters returns"""
        return self._export_staged(self.lib.w3_export_counters_staged, model, data)

    def export_profile(self):
        """w3_export_get_profile: what the last export_counters_device / _staged call did (the times under set_timing())"""
        p = L.ExportProfile()
        self._chk(self.lib.w3_export_get_profile(self.h, C.byref(p)))
        return {k: getattr(p, k) for k, _ in L.ExportProfile._fields_}

    def export_entropy_device(self, model, d_in, d_counters=None, stream=None):
        """w3_export_entropy_device: export_counters_device for ONE adaptive leaf with any history — OrderN, or OrderNEntropy over
        RawHistory, ACHistory or HuffHistory (init_model()'s leaf) — with a key stage per epoch (csrc/w3_export_entropy.h).  d_in: a
        torch.uint8 CUDA tensor (contiguous).  -> a torch.int32 CUDA tensor of 2^bits packed counters n0 | n1 << 16 (d_counters when
        given: every entry is overwritten)"""
        return self._export_device(self.lib.w3_export_entropy_device, model, d_in, d_counters, stream)

    def export_entropy_staged(self, model, data):
        """w3_export_entropy_staged: the same from host `data` of any length, staged through the device in pieces.
        -> (n0: np.uint16[2^bits], n1: np.uint16[2^bits]), the shape export_counters returns"""
        return self._export_staged(self.lib.w3_export_entropy_staged, model, data)

    def export_entropy_profile(self):
        """w3_export_entropy_get_profile: what the last export_entropy_device / _staged call did (the times under set_timing()):
        export_profile()'s fields, key_ms and huff_fixed_epochs"""
        p = L.ExportEntropyProfile()
        self._chk(self.lib.w3_export_entropy_get_profile(self.h, C.byref(p)))
        out = {k: getattr(p.base, k) for k, _ in L.ExportProfile._fields_}
        out.update(key_ms=p.key_ms, huff_fixed_epochs=p.huff_fixed_epochs)
        return out

    # ---- which kernels decode (include/w3hip.h "which kernels decode") ----
    @staticmethod
    def decode_spec_covers(model, variant=()):
        """w3_decode_spec_covers: whether the sixteen-lane decoder takes a decode of this model under default options (False: the
        lane-per-block kernels do) — or, with `variant` (set_variant's names), w3_decode_spec_covers_variant: under those variant bits,
        e.g. ("decode_match_spec",) for a model with a match-model leaf.  Host only: needs no context and no device.  A spec the
        library refuses raises W3Error."""
        spec = model.spec() if isinstance(model, Model) else model
        if variant:
            rc = L.load().w3_decode_spec_covers_variant(C.byref(spec), Context.variant_bits(variant))
        else:
            rc = L.load().w3_decode_spec_covers(C.byref(spec))
        if rc < 0:
            raise W3Error(rc, "w3_decode_spec_covers: the spec is refused")
        return bool(rc)

    def last_decode_path(self):
        """w3_last_decode_path: L.W3_PATH_SPEC or L.W3_PATH_GENERIC, the kernel family this context's most recent decode_blocks* /
        decode_ranges* call launched; 0 before any decode"""
        return int(self.lib.w3_last_decode_path(self.h))

    # ---- per-step statistics (include/w3hip.h "per-step statistics"; csrc/w3_steps.h) ----
    _STEPS_FORMATS = {"p_u16": L.W3_STEPS_P_U16, "stretch_i16": L.W3_STEPS_STRETCH_I16, "stretch_f16": L.W3_STEPS_STRETCH_F16}
    _STEPS_NUMPY = {"p_u16": np.uint16, "stretch_i16": np.int16, "stretch_f16": np.float16}

    @staticmethod
    def steps_layout(model, format="stretch_f16", bit=False):
        """w3_steps_layout_of: the columns of a row of export_steps* for this model -> dict(n_cols, n_leaves, col_mix, col_apm0, n_apm,
        col_final, col_bit, elem_bytes); col_apm0 / col_bit are None where there is no such column.  Host only: needs no context
        (Context.steps_layout(model, ...)) and no device."""
        spec = model.spec() if isinstance(model, Model) else model
        lay = L.StepsLayout()
        # (a format or flags value given as a number goes through as it is: the library refuses what it does not know)
        fmt = Context._STEPS_FORMATS.get(format, 0xFFFF) if isinstance(format, str) else int(format)
        flags = (L.W3_STEPS_COL_BIT if bit else 0) if isinstance(bit, bool) else int(bit)
        rc = L.load().w3_steps_layout_of(C.byref(spec), fmt, flags, C.byref(lay))
        if rc:
            raise W3Error(rc, "w3_steps_layout_of: malformed spec, or an unknown format or flag")
        out = {k: getattr(lay, k) for k, _ in L.StepsLayout._fields_}
        for k in ("col_apm0", "col_bit"):
            if out[k] == L.W3_STEPS_NO_COL:
                out[k] = None
        return out

    @staticmethod
    def _steps_format(format):
        """the export calls take a format by NAME (steps_layout also passes numbers through, for the library to refuse)"""
        if not isinstance(format, str) or format not in Context._STEPS_FORMATS:
            raise W3Error(L.W3_E_INVALID, "format: one of %s" % ", ".join(sorted(Context._STEPS_FORMATS)))
        return Context._STEPS_FORMATS[format]

    @staticmethod
    def _probs_args(d_in, d_p):
        import torch
        if d_in.dtype != torch.uint8 or not d_in.is_cuda or not d_in.is_contiguous():
            raise W3Error(L.W3_E_INVALID, "d_in: a contiguous torch.uint8 CUDA tensor")
        if d_p.numel() != 8 * d_in.numel() or d_p.element_size() != 2 or not d_p.is_contiguous() or d_p.device != d_in.device:
            raise W3Error(L.W3_E_INVALID, "d_p: a contiguous tensor of 8 n 16-bit values on d_in's device")

    @staticmethod
    def _steps_torch_dtype(format):
        import torch
        if format == "p_u16":
            return getattr(torch, "uint16", torch.int16)
        return torch.int16 if format == "stretch_i16" else torch.float16

    def export_steps_device(self, model, d_in, block_size, format="stretch_f16", bit=True, out=None, stream=None):
        """w3_export_steps_device: one row per coded bit of what every part of the model said before it — a column per leaf, the mix, a
        column per APM stage, and (bit=True) the coded bit; steps_layout() names the columns.  d_in: a contiguous torch.uint8 CUDA
        tensor; the bytes never leave the device.  format: "p_u16" (Counter::p as is), "stretch_i16" (stretch[p >> 4], -2047 .. 2047),
        "stretch_f16" (that / 256, exact).  -> a CUDA tensor [8 n, C] of torch.uint16 / int16 / float16 (`out` when given: a contiguous
        tensor of that shape and dtype on d_in's device).  Where this torch build has no uint16, "p_u16" rows come as torch.int16
        holding the same bits."""
        import torch
        if d_in.dtype != torch.uint8 or not d_in.is_cuda or not d_in.is_contiguous():
            raise W3Error(L.W3_E_INVALID, "d_in: a contiguous torch.uint8 CUDA tensor")
        fmt = self._steps_format(format)
        spec = model.spec() if isinstance(model, Model) else model
        lay = self.steps_layout(spec, format, bool(bit))
        n, cols, dt = d_in.numel(), lay["n_cols"], self._steps_torch_dtype(format)
        if out is None:
            out = torch.empty((8 * n, cols), dtype=dt, device=d_in.device)
        elif out.dtype != dt or tuple(out.shape) != (8 * n, cols) or not out.is_contiguous() or out.device != d_in.device:
            raise W3Error(L.W3_E_INVALID, "out: a contiguous %s tensor of shape (%d, %d) on d_in's device" % (dt, 8 * n, cols))
        st = C.c_void_p(stream) if stream else None
        self._chk(self.lib.w3_export_steps_device(self.h, C.byref(spec), C.c_void_p(d_in.data_ptr()), n, block_size, fmt,
                                                  L.W3_STEPS_COL_BIT if bit else 0, C.c_void_p(out.data_ptr()), out.numel() * 2, st))
        return out

    def export_steps(self, model, data, block_size, format="stretch_f16", bit=True):
        """w3_export_steps_staged: the same rows from host `data` of any length, through the device in pieces of whole blocks
        (set_host_chunk_blocks).  -> np.ndarray [8 n, C] of uint16 / int16 / float16"""
        fmt = self._steps_format(format)
        spec = model.spec() if isinstance(model, Model) else model
        lay = self.steps_layout(spec, format, bool(bit))
        a = _u8(data)
        rows = np.empty((8 * len(a), lay["n_cols"]), dtype=self._STEPS_NUMPY[format])
        self._chk(self.lib.w3_export_steps_staged(self.h, C.byref(spec), a.ctypes.data_as(C.c_void_p), len(a), block_size, fmt,
                                                  L.W3_STEPS_COL_BIT if bit else 0, rows.ctypes.data_as(C.c_void_p), rows.nbytes))
        return rows

    def iter_steps(self, model, d_in, block_size, blocks_per_batch, format="stretch_f16", bit=True, stream=None):
        """export_steps_device in batches of `blocks_per_batch` whole blocks — a workload's rows do not fit one tensor (1e9 bytes x 6
        columns is 96 GB).  Yields (first_step, rows): rows is a view of ONE reused tensor (consume or copy it before the next batch),
        rows[j] is step first_step + j."""
        n, run = d_in.numel(), int(blocks_per_batch) * int(block_size)
        if run <= 0:
            raise W3Error(L.W3_E_INVALID, "blocks_per_batch and block_size must be positive")
        buf = None
        for o0 in range(0, n, run):
            piece = d_in[o0:o0 + run]
            if buf is None:
                buf = self.export_steps_device(model, piece, block_size, format, bit, stream=stream)
                rows = buf
            else:
                rows = self.export_steps_device(model, piece, block_size, format, bit, out=buf[:8 * piece.numel()], stream=stream)
            yield 8 * o0, rows

    def steps_profile(self):
        """w3_export_steps_get_profile: what the last export_steps* call did (the times under set_timing())"""
        p = L.StepsProfile()
        self._chk(self.lib.w3_export_steps_get_profile(self.h, C.byref(p)))
        return {k: getattr(p, k) for k, _ in L.StepsProfile._fields_}

    def encode_probs_device(self, d_in, block_size, d_p, out_cap=None, stream=None):
        """w3_encode_probs_device: the block container's streams with the caller's probabilities in place of a model's — d_p: a
        contiguous CUDA tensor of 8 n 16-bit values (uint16, or int16 holding the same bits; 16-byte aligned), d_p[8 i + k] = P(bit k of
        byte i is 1), each in 1 .. 65535 (a zero is refused: W3_E_INVALID names the first such step).  -> (out: torch.uint8 CUDA tensor of
        the concatenated streams, block_lens: torch.int32 [nb]).  There is no decode counterpart."""
        import torch
        self._probs_args(d_in, d_p)
        n = d_in.numel()
        nb = (n + block_size - 1) // block_size if block_size else 0
        cap = int(out_cap) if out_cap is not None else int(self.lib.w3_max_compressed_size(n, block_size))
        out = torch.empty(max(cap, 1), dtype=torch.uint8, device=d_in.device)
        lens = torch.zeros(max(nb, 1), dtype=torch.int32, device=d_in.device)
        total = torch.zeros(1, dtype=torch.int64, device=d_in.device)
        st = C.c_void_p(stream) if stream else None
        self._chk(self.lib.w3_encode_probs_device(self.h, C.c_void_p(d_in.data_ptr()), n, block_size, C.c_void_p(d_p.data_ptr()),
                                                  C.c_void_p(out.data_ptr()), cap, C.c_void_p(lens.data_ptr()), C.c_void_p(total.data_ptr()), st))
        return out[: int(total.item())], lens[:nb]

    def encode_stats_probs_device(self, d_in, block_size, d_p, stream=None):
        """w3_encode_stats_probs_device: the ACStats bit counts (encode_stats) of the same coding -> torch.int32 [nb] CUDA tensor"""
        import torch
        self._probs_args(d_in, d_p)
        n = d_in.numel()
        nb = (n + block_size - 1) // block_size if block_size else 0
        bits = torch.zeros(max(nb, 1), dtype=torch.int32, device=d_in.device)
        st = C.c_void_p(stream) if stream else None
        self._chk(self.lib.w3_encode_stats_probs_device(self.h, C.c_void_p(d_in.data_ptr()), n, block_size, C.c_void_p(d_p.data_ptr()),
                                                        C.c_void_p(bits.data_ptr()), st))
        return bits[:nb]

    def predict_blocks(self, model, data, block_size):
        spec = model.spec()
        a = _u8(data)
        p = np.empty(max(len(a) * 8, 1), dtype=np.uint16)
        self._chk(self.lib.w3_predict_blocks(self.h, C.byref(spec), a.ctypes.data_as(C.c_void_p), len(a), block_size,
                                             p.ctypes.data_as(C.c_void_p)))
        return p[: len(a) * 8]

    # ---- AC over Huffman (bin/ac-over-huffman/main.rs:46-89; include/w3hip.h w3_aoh_*) ----
    def aoh_encode_blocks(self, code, ctx_bits, data, block_size, out_cap=None):
        """OrderN(ctx_bits, 0) over the bits of the bytes' Huffman codes (`code`: a HuffCode), block container.
        -> (concatenated streams: np.uint8[], block_lens: np.uint32[])"""
        a = _u8(data)
        n = len(a)
        nb = (n + block_size - 1) // block_size if block_size else 0
        if out_cap is None:
            out_cap = 2 * n + 64 * nb + 64
        while True:
            out = np.empty(max(out_cap, 1), dtype=np.uint8)
            lens = np.zeros(max(nb, 1), dtype=np.uint32)
            olen = C.c_size_t()
            rc = self.lib.w3_aoh_encode_blocks(self.h, C.byref(code.table), ctx_bits, a.ctypes.data_as(C.c_void_p), n, block_size,
                                               out.ctypes.data_as(C.c_void_p), out_cap, C.byref(olen), lens.ctypes.data_as(C.c_void_p))
            if rc == L.W3_E_NOSPACE and olen.value > out_cap:
                out_cap = olen.value
                continue
            self._chk(rc)
            return out[: olen.value], lens[:nb]

    def aoh_decode_blocks(self, code, ctx_bits, comp, block_lens, block_size, orig_len, crc=None):
        """crc: as decode_blocks (w3_aoh_decode_blocks_checked)"""
        a = _u8(comp)
        lens = np.ascontiguousarray(block_lens, dtype=np.uint32)
        out = np.empty(max(orig_len, 1), dtype=np.uint8)
        args = (self.h, C.byref(code.table), ctx_bits, a.ctypes.data_as(C.c_void_p), len(a), lens.ctypes.data_as(C.c_void_p),
                len(lens), block_size, orig_len, out.ctypes.data_as(C.c_void_p))
        if crc is None:
            self._chk(self.lib.w3_aoh_decode_blocks(*args))
        else:
            ck, _keep = self._check(crc)
            self._chk(self.lib.w3_aoh_decode_blocks_checked(*args, C.byref(ck)), ck)
        return out[:orig_len]

    def aoh_decode_ranges(self, code, ctx_bits, comp, block_lens, block_size, orig_len, ranges, crc=None):
        """Random access on AC-over-Huffman streams (w3_aoh_decode_ranges): the bytes of `ranges` — (offset, len) pairs or an (n, 2) integer
        array — of the original data, concatenated in request order, decoding only the blocks they touch.  -> np.uint8[sum of the lengths]
        crc: as decode_ranges (w3_aoh_decode_ranges_checked)"""
        a = _u8(comp)
        lens = np.ascontiguousarray(block_lens, dtype=np.uint32)
        rs, n, total = _ranges(ranges)
        out = np.empty(max(total, 1), dtype=np.uint8)
        olen = C.c_size_t()
        args = (self.h, C.byref(code.table), ctx_bits, a.ctypes.data_as(C.c_void_p), len(a), lens.ctypes.data_as(C.c_void_p),
                len(lens), block_size, orig_len, rs, n, out.ctypes.data_as(C.c_void_p), total, C.byref(olen))
        if crc is None:
            self._chk(self.lib.w3_aoh_decode_ranges(*args))
        else:
            ck, _keep = self._check(crc)
            self._chk(self.lib.w3_aoh_decode_ranges_checked(*args, C.byref(ck)), ck)
        return out[: olen.value]

    def aoh_decode_spec_covers(self, ctx_bits):
        """w3_aoh_decode_spec_covers: whether the sixteen-lane decoder takes a call with this ctx_bits"""
        return bool(self.lib.w3_aoh_decode_spec_covers(int(ctx_bits)))

    def aoh_encode_stats(self, code, ctx_bits, data, block_size):
        """ACStats bit counts per block (what the driver's csize = bits / 8 comes from, :72, :88).  -> np.uint32[nb]"""
        a = _u8(data)
        nb = (len(a) + block_size - 1) // block_size if block_size else 0
        bits = np.zeros(max(nb, 1), dtype=np.uint32)
        self._chk(self.lib.w3_aoh_encode_stats(self.h, C.byref(code.table), ctx_bits, a.ctypes.data_as(C.c_void_p), len(a), block_size,
                                               bits.ctypes.data_as(C.c_void_p)))
        return bits[:nb]

    @staticmethod
    def _aoh_cfgs(codes, configs):
        tabs = (L.HuffCode * max(len(codes), 1))(*[c.table for c in codes])
        ci = np.array([c[0] for c in configs], dtype=np.uint8)
        cb = np.array([c[1] for c in configs], dtype=np.uint8)
        return tabs, ci, cb

    def sweep_ac_over_huffman(self, data, block_size, codes, configs):
        """The driver's sweep (:20-32) in one call: `codes` = HuffCode list, `configs` = (index into codes, ctx_bits) pairs.
        -> np.uint32[len(configs)][nb] ACStats bit counts."""
        a = _u8(data)
        nb = (len(a) + block_size - 1) // block_size if block_size else 0
        tabs, ci, cb = self._aoh_cfgs(codes, configs)
        out = np.zeros((len(configs), max(nb, 1)), dtype=np.uint32)
        self._chk(self.lib.w3_sweep_ac_over_huffman(self.h, a.ctypes.data_as(C.c_void_p), len(a), block_size, tabs, len(codes),
                                                    ci.ctypes.data_as(C.c_void_p), cb.ctypes.data_as(C.c_void_p), len(configs),
                                                    out.ctypes.data_as(C.c_void_p)))
        return out[:, :nb]

    def aoh_compress(self, data, huffman_size=13, ctx_bits=24, block_size=65536):
        """Container writer's form: the table of `data` (HuffCode.new_on: the histogram is taken on the device), encode.  A one-symbol input gives the all-zero table, as in the
        reference, where such a file codes zero bits; it is turned into len 1, code 0 for that symbol HERE, before encoding, so that
        the streams can be decoded.  -> (HuffCode used, streams, block_lens)"""
        a = _u8(data)
        code = HuffCode.new_on(self, a, huffman_size)
        if len(a) and not any(code.lens):
            code = code.with_single_symbol(int(a[0]))
        out, lens = self.aoh_encode_blocks(code, ctx_bits, a, block_size)
        return code, out, lens

    # ---- reference container (main.rs:89-144) ------------------------------
    def compress(self, data, model=None):
        """compress(): b"w30i" + u64 BE len + one stream."""
        model = model or init_model()
        spec = model.spec()
        a = _u8(data)
        cap = 2 * len(a) + 128
        while True:
            out = np.empty(cap, dtype=np.uint8)
            olen = C.c_size_t()
            rc = self.lib.w3_compress_stream(self.h, C.byref(spec), a.ctypes.data_as(C.c_void_p), len(a),
                                             out.ctypes.data_as(C.c_void_p), cap, C.byref(olen))
            if rc == L.W3_E_NOSPACE and olen.value > cap:
                cap = olen.value
                continue
            self._chk(rc)
            return out[: olen.value].tobytes()

    def decompress(self, data, model=None):
        model = model or init_model()
        spec = model.spec()
        a = _u8(data)
        if len(a) >= 12 and a[:4].tobytes() == MAGIC_STR:
            n = int.from_bytes(a[4:12].tobytes(), "big")
        else:
            n = 0
        out = np.empty(max(n, 1), dtype=np.uint8)
        olen = C.c_size_t()
        rc = self.lib.w3_decompress_stream(self.h, C.byref(spec), a.ctypes.data_as(C.c_void_p), len(a),
                                           out.ctypes.data_as(C.c_void_p), n, C.byref(olen))
        self._chk(rc)
        return out[: olen.value].tobytes()

    # ---- device-resident (torch tensors own the memory) ------------------------
    def encode_blocks_device(self, model, d_in, block_size, d_out, d_lens, d_total, stream=None):
        """d_in/d_out: torch.uint8 CUDA tensors, d_lens: int32/uint32[nb], d_total: int64[1].  Returns rc-checked None."""
        spec = model.spec() if isinstance(model, Model) else model
        # stream: a hipStream_t handle as an int.  None or 0 = the ctx's own (blocking) stream, which is ordered against the
        # legacy default stream — torch's default stream IS that stream (handle 0), so both spellings mean the same order.
        st = C.c_void_p(stream) if stream else None
        rc = self.lib.w3_encode_blocks_device(self.h, C.byref(spec), C.c_void_p(d_in.data_ptr()), d_in.numel(), block_size,
                                              C.c_void_p(d_out.data_ptr()), d_out.numel(), C.c_void_p(d_lens.data_ptr()),
                                              C.c_void_p(d_total.data_ptr()), st)
        self._chk(rc)

    def encode_submit(self, model, d_in, block_size, d_out, d_lens, d_total, stream=None):
        """w3_encode_submit: enqueue the encode and return a job handle at once (at most max_in_flight(n, block_size, model) jobs in
        flight: four up to 4,096 blocks, three up to 12,288, two beyond; the next call's predict phase runs beside this call's APM and
        coder kernels).  Keep every tensor alive and untouched until encode_wait(job)."""
        spec = model.spec() if isinstance(model, Model) else model
        st = C.c_void_p(stream) if stream else None
        job = C.c_int(-1)
        rc = self.lib.w3_encode_submit(self.h, C.byref(spec), C.c_void_p(d_in.data_ptr()), d_in.numel(), block_size,
                                       C.c_void_p(d_out.data_ptr()), d_out.numel(), C.c_void_p(d_lens.data_ptr()),
                                       C.c_void_p(d_total.data_ptr()), st, C.byref(job))
        self._chk(rc)
        return job.value

    def max_in_flight(self, n, block_size, model=None):
        """w3_encode_max_in_flight: submitted calls of this size one context keeps in flight (4 up to 4,096 blocks, 3 up to 12,288, else 2;
        models with slot-state leaves: 2)."""
        spec = None if model is None else (model.spec() if isinstance(model, Model) else model)
        return int(self.lib.w3_encode_max_in_flight(C.byref(spec) if spec is not None else None, int(n), int(block_size)))

    def encode_wait(self, job):
        """w3_encode_wait: block until the job's output is complete (raises what the synchronous call would have raised)."""
        self._chk(self.lib.w3_encode_wait(self.h, int(job)))

    def decode_blocks_device(self, model, d_comp, d_lens, block_size, orig_len, d_out, stream=None):
        spec = model.spec() if isinstance(model, Model) else model
        st = C.c_void_p(stream) if stream else None
        rc = self.lib.w3_decode_blocks_device(self.h, C.byref(spec), C.c_void_p(d_comp.data_ptr()), d_comp.numel(), C.c_void_p(d_lens.data_ptr()),
                                              d_lens.numel(), block_size, orig_len, C.c_void_p(d_out.data_ptr()), st)
        self._chk(rc)

    def decode_ranges_device(self, model, d_comp, d_lens, block_size, orig_len, ranges, d_out, stream=None, crc=None):
        """w3_decode_ranges_device: the bytes of `ranges` ((offset, len) pairs or an (n, 2) integer array, host side) of the original data,
        concatenated in request order into the torch.uint8 CUDA tensor d_out.  -> bytes written
        crc: the CRC-32 table of all the container's blocks, HOST side (w3_decode_ranges_device_checked)"""
        spec = model.spec() if isinstance(model, Model) else model
        st = C.c_void_p(stream) if stream else None
        rs, n, _ = _ranges(ranges)
        olen = C.c_size_t()
        args = (self.h, C.byref(spec), C.c_void_p(d_comp.data_ptr()), d_comp.numel(), C.c_void_p(d_lens.data_ptr()),
                d_lens.numel(), block_size, orig_len, rs, n, C.c_void_p(d_out.data_ptr()), d_out.numel(), C.byref(olen), st)
        if crc is None:
            self._chk(self.lib.w3_decode_ranges_device(*args))
        else:
            ck, _keep = self._check(crc)
            self._chk(self.lib.w3_decode_ranges_device_checked(*args, C.byref(ck)), ck)
        return olen.value


    def aoh_encode_blocks_device(self, code, ctx_bits, d_in, block_size, d_out, d_lens, d_total, stream=None):
        """w3_aoh_encode_blocks_device: tensors as encode_blocks_device."""
        st = C.c_void_p(stream) if stream else None
        self._chk(self.lib.w3_aoh_encode_blocks_device(self.h, C.byref(code.table), ctx_bits, C.c_void_p(d_in.data_ptr()), d_in.numel(), block_size,
                                                       C.c_void_p(d_out.data_ptr()), d_out.numel(), C.c_void_p(d_lens.data_ptr()),
                                                       C.c_void_p(d_total.data_ptr()), st))

    def aoh_decode_blocks_device(self, code, ctx_bits, d_comp, d_lens, block_size, orig_len, d_out, stream=None):
        st = C.c_void_p(stream) if stream else None
        self._chk(self.lib.w3_aoh_decode_blocks_device(self.h, C.byref(code.table), ctx_bits, C.c_void_p(d_comp.data_ptr()), d_comp.numel(),
                                                       C.c_void_p(d_lens.data_ptr()), d_lens.numel(), block_size, orig_len,
                                                       C.c_void_p(d_out.data_ptr()), st))

    def aoh_decode_ranges_device(self, code, ctx_bits, d_comp, d_lens, block_size, orig_len, ranges, d_out, stream=None, crc=None):
        """w3_aoh_decode_ranges_device: the bytes of `ranges` (host side, as aoh_decode_ranges) concatenated in request order into the
        torch.uint8 CUDA tensor d_out.  -> bytes written.  crc: as decode_ranges_device (w3_aoh_decode_ranges_device_checked)"""
        st = C.c_void_p(stream) if stream else None
        rs, n, _ = _ranges(ranges)
        olen = C.c_size_t()
        args = (self.h, C.byref(code.table), ctx_bits, C.c_void_p(d_comp.data_ptr()), d_comp.numel(),
                C.c_void_p(d_lens.data_ptr()), d_lens.numel(), block_size, orig_len, rs, n,
                C.c_void_p(d_out.data_ptr()), d_out.numel(), C.byref(olen), st)
        if crc is None:
            self._chk(self.lib.w3_aoh_decode_ranges_device(*args))
        else:
            ck, _keep = self._check(crc)
            self._chk(self.lib.w3_aoh_decode_ranges_device_checked(*args, C.byref(ck)), ck)
        return olen.value

    def aoh_encode_stats_device(self, code, ctx_bits, d_in, block_size, d_bits, stream=None):
        """d_bits: int32/uint32[nb] CUDA tensor receiving the ACStats bit counts."""
        st = C.c_void_p(stream) if stream else None
        self._chk(self.lib.w3_aoh_encode_stats_device(self.h, C.byref(code.table), ctx_bits, C.c_void_p(d_in.data_ptr()), d_in.numel(), block_size,
                                                      C.c_void_p(d_bits.data_ptr()), st))

    def sweep_ac_over_huffman_device(self, d_in, block_size, codes, configs):
        """sweep_ac_over_huffman on a torch.uint8 CUDA tensor.  -> np.uint32[len(configs)][nb] (host)"""
        n = d_in.numel()
        nb = (n + block_size - 1) // block_size if block_size else 0
        tabs, ci, cb = self._aoh_cfgs(codes, configs)
        out = np.zeros((len(configs), max(nb, 1)), dtype=np.uint32)
        self._chk(self.lib.w3_sweep_ac_over_huffman_device(self.h, C.c_void_p(d_in.data_ptr()), n, block_size, tabs, len(codes),
                                                           ci.ctypes.data_as(C.c_void_p), cb.ctypes.data_as(C.c_void_p), len(configs),
                                                           out.ctypes.data_as(C.c_void_p)))
        return out[:, :nb]


AOH_CONTAINER_MAGIC = b"w3bk\x02"   # tools/w3cli.cpp: the block container, version 2 (AC over Huffman)


def aoh_container_ranges(ctx, blob, ranges):
    """The bytes of `ranges` of a version-2 `w3bk` container (an AC-over-Huffman file as tools/w3cli.cpp writes it: magic, version 2,
    u64 original length, u32 block size, u32 block count, ctx_bits, the 256 codes (u16) and lengths (u8), the u32 length table — all
    big-endian — then the streams), through Context.aoh_decode_ranges.  W3Error(W3_E_FORMAT) for anything else."""
    a = _u8(blob)
    hdr = 21 + 1 + 768
    if len(a) < 21 or a[:5].tobytes() != AOH_CONTAINER_MAGIC:
        raise W3Error(L.W3_E_FORMAT, "not a version-2 w3bk container")
    orig, bs, nb = int.from_bytes(a[5:13].tobytes(), "big"), int.from_bytes(a[13:17].tobytes(), "big"), int.from_bytes(a[17:21].tobytes(), "big")
    if bs == 0 or nb != (orig + bs - 1) // bs or len(a) < hdr + 4 * nb:
        raise W3Error(L.W3_E_FORMAT, "truncated or inconsistent w3bk header")
    ctx_bits = int(a[21])
    codes = a[22:22 + 512].view(">u2").astype(np.uint16).tolist()
    lens = a[22 + 512:22 + 768].tolist()
    block_lens = a[hdr:hdr + 4 * nb].view(">u4").astype(np.uint32)
    comp = a[hdr + 4 * nb:]
    if int(block_lens.sum(dtype=np.uint64)) > len(comp):
        raise W3Error(L.W3_E_FORMAT, "the w3bk length table claims more than the file holds")
    return ctx.aoh_decode_ranges(HuffCode.from_tables(codes, lens), ctx_bits, comp, block_lens, bs, orig, ranges)


def encode_blocks_sharded_device(ctxs, model, d_ins, block_size, d_out, d_lens, root=0, transport="auto"):
    """w3_encode_blocks_sharded_device: ONE process, one Context per device; d_ins[r] (torch.uint8 CUDA tensor on ctxs[r]'s device) is
    shard r of one stream (w3_shard_range); the packed streams and the length table are gathered on ctxs[root]'s device (d_out,
    d_lens) with RCCL (grouped send/recv over xGMI) or device copies.  -> per-shard compressed byte counts."""
    spec = model.spec() if isinstance(model, Model) else model
    k = len(ctxs)
    hs = (C.c_void_p * k)(*[c.h for c in ctxs])
    ins = (C.c_void_p * k)(*[C.c_void_p(t.data_ptr() if t.numel() else 0) for t in d_ins])
    ns = (C.c_size_t * k)(*[t.numel() for t in d_ins])
    totals = (C.c_uint64 * k)()
    tr = {"auto": L.W3_GATHER_AUTO, "rccl": L.W3_GATHER_RCCL, "peer_copy": L.W3_GATHER_PEER_COPY}[transport]
    rc = ctxs[0].lib.w3_encode_blocks_sharded_device(hs, k, C.byref(spec), ins, ns, block_size, root, C.c_void_p(d_out.data_ptr()), d_out.numel(),
                                                     C.c_void_p(d_lens.data_ptr()), totals, tr)
    if rc:
        raise W3Error(rc, ctxs[0].lib.w3_last_error(ctxs[0].h).decode())
    return [int(t) for t in totals]


def encode_sharded_submit(ctxs, model, d_ins, block_size):
    """w3_encode_sharded_submit: one STEP of a stream of sharded encodes — every shard's encode is enqueued on its context (d_ins[r]:
    torch.uint8 CUDA tensor on ctxs[r]'s device, kept alive until the step has been waited for).  -> step handle"""
    spec = model.spec() if isinstance(model, Model) else model
    k = len(ctxs)
    hs = (C.c_void_p * k)(*[c.h for c in ctxs])
    ins = (C.c_void_p * k)(*[C.c_void_p(t.data_ptr() if t.numel() else 0) for t in d_ins])
    ns = (C.c_size_t * k)(*[t.numel() for t in d_ins])
    sjob = C.c_int(-1)
    rc = ctxs[0].lib.w3_encode_sharded_submit(hs, k, C.byref(spec), ins, ns, block_size, C.byref(sjob))
    if rc:
        raise W3Error(rc, ctxs[0].lib.w3_last_error(ctxs[0].h).decode())
    return sjob.value


def encode_sharded_wait(ctxs, sjob, d_out, d_lens, root=0, transport="auto"):
    """w3_encode_sharded_wait: completes the step and gathers its packed streams and length table on ctxs[root]'s device.
    -> per-shard compressed byte counts"""
    k = len(ctxs)
    hs = (C.c_void_p * k)(*[c.h for c in ctxs])
    totals = (C.c_uint64 * k)()
    tr = {"auto": L.W3_GATHER_AUTO, "rccl": L.W3_GATHER_RCCL, "peer_copy": L.W3_GATHER_PEER_COPY}[transport]
    rc = ctxs[0].lib.w3_encode_sharded_wait(hs, k, int(sjob), root, C.c_void_p(d_out.data_ptr()), d_out.numel(), C.c_void_p(d_lens.data_ptr()), totals, tr)
    if rc:
        raise W3Error(rc, ctxs[0].lib.w3_last_error(ctxs[0].h).decode())
    return [int(t) for t in totals]


def sharded_max_in_flight(ctxs, model, sizes, block_size):
    spec = model.spec() if isinstance(model, Model) else model
    ns = (C.c_size_t * len(sizes))(*sizes)
    return int(ctxs[0].lib.w3_encode_sharded_max_in_flight(C.byref(spec), ns, len(sizes), block_size))
