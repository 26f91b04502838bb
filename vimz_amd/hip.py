"""Thin object wrapper over the C ABI (include/vimz_hip.h) for Python callers: tests, bench.py and the
host-side folding driver.  Arrays are numpy uint64 with 4 limbs per field element; nothing is computed here.
"""
import ctypes as C

import numpy as np

from . import _lib as L


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


class DeviceVec:
    def __init__(self, ctx, handle, field, n):
        self.ctx, self.h, self.field, self.n = ctx, handle, field, n

    def upload(self, host, offset=0, form=L.FORM_CANONICAL):
        host = _u64(host)
        self.ctx._chk(self.ctx.lib.vimz_vec_upload(self.ctx.h, self.h, offset, _ptr(host), host.size // 4, form))
        return self

    def download(self, offset=0, n=None, form=L.FORM_CANONICAL):
        n = self.n - offset if n is None else n
        out = np.zeros((n, 4), dtype=np.uint64)
        self.ctx._chk(self.ctx.lib.vimz_vec_download(self.ctx.h, self.h, offset, _ptr(out), n, form))
        return out

    def free(self):
        if self.h:
            self.ctx.lib.vimz_vec_free(self.ctx.h, self.h)
            self.h = None


class Bases:
    def __init__(self, ctx, handle, curve, n):
        self.ctx, self.h, self.curve, self.n = ctx, handle, curve, n

    def precompute(self, window_bits=0):
        """Window tables in HBM (vimz_bases_precompute): later MSMs over this key share one bucket set."""
        self.ctx._chk(self.ctx.lib.vimz_bases_precompute(self.ctx.h, self.h, window_bits))
        return self

    def download(self, offset=0, n=None, form=L.FORM_CANONICAL):
        n = self.n - offset if n is None else n
        out = np.zeros((n, 8), dtype=np.uint64)
        self.ctx._chk(self.ctx.lib.vimz_bases_download(self.ctx.h, self.h, offset, _ptr(out), n, form))
        return out

    def free(self):
        if self.h:
            self.ctx.lib.vimz_bases_free(self.ctx.h, self.h)
            self.h = None


class ImageDesc(C.Structure):
    """vimz_image_desc (include/vimz_hip.h)."""
    _fields_ = [("pixels", C.c_void_p), ("height", C.c_size_t), ("width", C.c_size_t), ("channels", C.c_int),
                ("units", C.c_void_p), ("n_units", C.c_size_t), ("unit_len", C.c_size_t), ("block", C.c_int),
                ("max_units", C.c_size_t), ("drop", C.c_void_p)]


_NO_FLAGS = np.zeros(1, dtype=np.uint8)       # a non-NULL address for an empty redact flag list

EDIT_OPS = {"hash": 0, "grayscale": 1, "brightness": 2, "contrast": 3, "blur": 4, "sharpness": 5, "resize": 6, "crop": 7, "redact": 8}


class EditDesc(C.Structure):
    """vimz_edit_desc (include/vimz_hip.h)."""
    _fields_ = [("op", C.c_int), ("pixels", C.c_void_p), ("height", C.c_size_t), ("width", C.c_size_t), ("channels", C.c_int),
                ("source", C.c_int64), ("factor", C.c_double), ("x", C.c_size_t), ("y", C.c_size_t), ("new_width", C.c_size_t),
                ("new_height", C.c_size_t), ("redact", C.c_void_p), ("n_redact", C.c_size_t), ("out_pixels", C.c_void_p),
                ("out_source", C.c_void_p), ("out_target", C.c_void_p)]


class EditShape(C.Structure):
    """vimz_edit_shape (include/vimz_hip.h)."""
    _fields_ = [("height", C.c_size_t), ("width", C.c_size_t), ("channels", C.c_int), ("source_units", C.c_size_t), ("source_unit_len", C.c_size_t),
                ("target_units", C.c_size_t), ("target_unit_len", C.c_size_t)]


class Context:
    """One per GPU (vimz_ctx)."""

    def __init__(self, device=0):
        self.lib = L.lib()
        h = C.c_void_p()
        rc = self.lib.vimz_ctx_create(device, C.byref(h))
        if rc != L.OK:
            raise L.VimzError(rc, self.lib.vimz_last_error(None).decode())
        self.h = h
        self.device = device

    def _chk(self, rc):
        if rc != L.OK:
            raise L.VimzError(rc, self.lib.vimz_last_error(self.h).decode())

    def close(self):
        if self.h:
            self.lib.vimz_ctx_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def device_info(self):
        name = C.create_string_buffer(256)
        cus, hbm = C.c_int(), C.c_uint64()
        self._chk(self.lib.vimz_device_info(self.h, name, 256, C.byref(cus), C.byref(hbm)))
        return {"name": name.value.decode(), "cus": cus.value, "hbm_bytes": hbm.value}

    def host_fingerprint(self):
        """vimz_host_fingerprint: what a benchmark line says about the HOST it was measured on."""
        out = (C.c_double * 4)()
        self.lib.vimz_host_fingerprint.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        self._chk(self.lib.vimz_host_fingerprint(self.h, out))
        model = "?"
        try:
            for line in open("/proc/cpuinfo"):
                if line.startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
        except OSError:
            pass
        return {"cpu_model": model, "us_per_host_poseidon_t9": out[0], "us_per_empty_launch_and_sync": out[1], "usable_cores": int(out[2]),
                "us_per_event_record_and_sync": out[3]}

    def trace_marker(self, ident):
        """vimz_trace_marker: an empty kernel of `ident` workgroups in the profiler's kernel trace (bench.py: 1 / 2 around the timed region)."""
        self.lib.vimz_trace_marker.argtypes = [C.c_void_p, C.c_int]
        self._chk(self.lib.vimz_trace_marker(self.h, int(ident)))

    def sync(self):
        self._chk(self.lib.vimz_sync(self.h))

    def timer_start(self):
        self._chk(self.lib.vimz_timer_start(self.h))

    def timer_stop(self):
        ms = C.c_float()
        self._chk(self.lib.vimz_timer_stop(self.h, C.byref(ms)))
        return ms.value

    def set_profiling(self, on):
        self._chk(self.lib.vimz_set_profiling(self.h, 1 if on else 0))

    def msm_last_profile(self):
        ms = (C.c_float * 6)()
        info = (C.c_uint32 * 4)()
        self._chk(self.lib.vimz_msm_last_profile(self.h, ms, info))
        names = ["hist", "scan", "scatter", "accumulate", "combine", "reduce"]
        return {"ms": dict(zip(names, list(ms))), "window_bits": info[0], "windows": info[1], "sub_buckets": info[2], "entries": info[3]}

    def msm_profile_totals(self, reset=False):
        self.lib.vimz_msm_profile_totals.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.c_int]
        ms = (C.c_double * 6)()
        cnt = (C.c_uint64 * 3)()
        self._chk(self.lib.vimz_msm_profile_totals(self.h, ms, cnt, 1 if reset else 0))
        names = ["hist", "scan", "scatter", "accumulate", "combine", "reduce"]
        return {"ms": dict(zip(names, list(ms))), "calls": int(cnt[0]), "points": int(cnt[1]), "entries": int(cnt[2])}

    # ---- commitment key / vectors
    def bases_upload(self, curve, xy, form=L.FORM_CANONICAL):
        xy = _u64(xy)
        n = xy.size // 8
        h = C.c_void_p()
        self._chk(self.lib.vimz_bases_upload(self.h, curve, _ptr(xy), n, form, C.byref(h)))
        return Bases(self, h, curve, n)

    def bases_generate(self, curve, n, label=b"ck"):
        h = C.c_void_p()
        self._chk(self.lib.vimz_bases_generate(self.h, curve, label, len(label), n, C.byref(h)))
        return Bases(self, h, curve, n)

    def vec_alloc(self, field, n):
        h = C.c_void_p()
        self._chk(self.lib.vimz_vec_alloc(self.h, field, n, C.byref(h)))
        return DeviceVec(self, h, field, n)

    def vec_from_host(self, field, host, form=L.FORM_CANONICAL):
        host = _u64(host)
        v = self.vec_alloc(field, host.size // 4)
        return v.upload(host, 0, form)

    # ---- input pipeline
    def pack_pixels(self, image, block=0):
        """compress_by_rows (block = 0) / compress_by_blocks (block = 40) of pyvimz on the device: (H, W[, 3]) uint8 ->
        (H, ceil(W/10), 4) or (blocks, block*block/10, 4) uint64 limbs."""
        img = np.ascontiguousarray(image, dtype=np.uint8)
        if img.ndim == 3 and img.shape[2] > 3:
            img = np.ascontiguousarray(img[:, :, :3])
        h, w = img.shape[:2]
        ch = 1 if img.ndim == 2 else 3
        lib = self.lib
        lib.vimz_pack_count.argtypes = [C.c_size_t, C.c_size_t, C.c_int]
        lib.vimz_pack_count.restype = C.c_size_t
        lib.vimz_pack_pixels.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
        n = lib.vimz_pack_count(h, w, block)
        out = np.zeros((n, 4), dtype=np.uint64)
        self._chk(lib.vimz_pack_pixels(self.h, _ptr(img), h, w, ch, block, _ptr(out)))
        if block:
            per = block * ((block + 9) // 10)
            return out.reshape(-1, per, 4)
        return out.reshape(h, -1, 4)

    def image_hash(self, descs):
        """vimz_image_hash over n images in one call.  descs: dicts with either `pixels` ((H, W) or (H, W, C) uint8, C = 1, 3 or 4) or `units`
        ((U, L, 4) uint64 canonical elements), and optionally `block` (0 / 40), `max_units`, `drop` (uint8 flags, one per hashed unit).
        Returns the n running hashes as ints.  (The arrays' lengths are the caller's to check: vimz_amd.image_hasher does.)"""
        n = len(descs)
        arr = (ImageDesc * n)()
        keep = []
        for i, d in enumerate(descs):
            D = arr[i]
            if d.get("pixels") is not None:
                px = np.ascontiguousarray(d["pixels"], dtype=np.uint8)
                keep.append(px)
                D.pixels = px.ctypes.data
                D.height, D.width = px.shape[0], px.shape[1]
                D.channels = 1 if px.ndim == 2 else px.shape[2]
            else:
                u = _u64(d["units"])
                keep.append(u)
                D.units = u.ctypes.data
                D.n_units, D.unit_len = u.shape[0], u.shape[1]
            D.block = int(d.get("block", 0))
            D.max_units = int(d.get("max_units", 0) or 0)
            if d.get("drop") is not None:
                dr = np.ascontiguousarray(d["drop"], dtype=np.uint8)
                keep.append(dr)
                D.drop = dr.ctypes.data
        out = np.zeros((n, 4), dtype=np.uint64)
        self.lib.vimz_image_hash.argtypes = [C.c_void_p, C.POINTER(ImageDesc), C.c_size_t, C.c_void_p]
        self._chk(self.lib.vimz_image_hash(self.h, arr, n, _ptr(out)))
        return [sum(int(r[k]) << (64 * k) for k in range(4)) for r in out]

    def image_hash_last_profile(self):
        """Milliseconds of the last image_hash call: {"digests": uploads + kernel + download, "chain": the host chains}."""
        ms = (C.c_double * 2)()
        self.lib.vimz_image_hash_last_profile.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        self._chk(self.lib.vimz_image_hash_last_profile(self.h, ms))
        return {"digests": ms[0], "chain": ms[1]}

    def image_edit(self, descs):
        """vimz_image_edit over n edit descriptors in one call, in order.  descs: dicts with
            op        a name of EDIT_OPS (or its number)
            pixels    the source, (H, W) or (H, W, C) uint8 with C = 1, 3 or 4 ... or
            source    the index of an earlier descriptor of the call, whose edited image (kept on the device) is the source
            factor, x, y, new_width, new_height, redact (uint8 flags, one per full 40 x 40 block)   the op's parameters
            want      the outputs to bring back, a subset of ("pixels", "source", "target") (default: all the op has)
        Returns one dict per descriptor {"pixels": (H', W'[, 3]) uint8, "source": (units, len, 4) uint64, "target": ...}, None where not wanted.
        (Arguments are checked by the library: a bad one raises VimzError(ERR_INVALID).)"""
        n = len(descs)
        arr = (EditDesc * n)()
        keep = []
        for i, d in enumerate(descs):
            D = arr[i]
            op = d.get("op")
            D.op = EDIT_OPS.get(op, -1) if isinstance(op, str) else int(op)
            if d.get("pixels") is not None:
                px = np.ascontiguousarray(d["pixels"], dtype=np.uint8)
                if px.ndim == 3 and px.shape[2] == 1:
                    px = px[:, :, 0]
                keep.append(px)
                D.pixels = px.ctypes.data
                D.height, D.width = px.shape[0], px.shape[1]
                D.channels = 1 if px.ndim == 2 else px.shape[2]
            else:
                D.source = int(d.get("source", -1))
            D.factor = float(d.get("factor") or 0.0)
            D.x, D.y = int(d.get("x") or 0), int(d.get("y") or 0)
            D.new_width, D.new_height = int(d.get("new_width") or 0), int(d.get("new_height") or 0)
            if d.get("redact") is not None:
                fl = np.ascontiguousarray(np.asarray(d["redact"]).reshape(-1) != 0, dtype=np.uint8)
                keep.append(fl)
                D.redact = fl.ctypes.data if fl.size else _NO_FLAGS.ctypes.data     # (never NULL: NULL asks for the checkerboard)
                D.n_redact = fl.size
        lib = self.lib
        lib.vimz_image_edit_shapes.argtypes = [C.c_void_p, C.POINTER(EditDesc), C.c_size_t, C.POINTER(EditShape)]
        lib.vimz_image_edit.argtypes = [C.c_void_p, C.POINTER(EditDesc), C.c_size_t]
        shapes = (EditShape * max(n, 1))()
        self._chk(lib.vimz_image_edit_shapes(self.h, arr, n, shapes))
        out = []
        dummy = np.zeros(4, dtype=np.uint64)       # (a packed output the op cannot give, e.g. redact's blocks of a 41 x 37 image: the library refuses it)
        for i, d in enumerate(descs):
            S, D = shapes[i], arr[i]
            want = d.get("want", ("pixels", "source", "target"))
            r = {"pixels": None, "source": None, "target": None}
            if "pixels" in want:
                r["pixels"] = np.empty((S.height, S.width) if S.channels == 1 else (S.height, S.width, S.channels), dtype=np.uint8)
                D.out_pixels = r["pixels"].ctypes.data
            if "source" in want:
                r["source"] = np.empty((S.source_units, S.source_unit_len, 4), dtype=np.uint64)
                D.out_source = r["source"].ctypes.data if r["source"].size else dummy.ctypes.data
            if "target" in want and D.op != EDIT_OPS["hash"]:
                r["target"] = np.empty((S.target_units, S.target_unit_len, 4), dtype=np.uint64)
                D.out_target = r["target"].ctypes.data if r["target"].size else dummy.ctypes.data
            out.append(r)
        self._chk(lib.vimz_image_edit(self.h, arr, n))
        return out

    def image_edit_last_profile(self):
        """Milliseconds of the last image_edit call: {"upload", "kernels", "download"}."""
        ms = (C.c_double * 3)()
        self.lib.vimz_image_edit_last_profile.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        self._chk(self.lib.vimz_image_edit_last_profile(self.h, ms))
        return {"upload": ms[0], "kernels": ms[1], "download": ms[2]}

    # ---- MSM
    def msm(self, bases, scalars, form=L.FORM_CANONICAL, window_bits=0, out_form=L.FORM_CANONICAL):
        scalars = _u64(scalars)
        out = np.zeros(8, dtype=np.uint64)
        self._chk(self.lib.vimz_msm(self.h, bases.h, _ptr(scalars), scalars.size // 4, form, window_bits, _ptr(out), out_form))
        return out

    def msm_vec(self, bases, vec, n=None, offset=0, base_offset=0, window_bits=0, out_form=L.FORM_CANONICAL, split_ones=False):
        n = vec.n - offset if n is None else n
        out = np.zeros(8, dtype=np.uint64)
        if split_ones:
            self._chk(self.lib.vimz_msm_vec_ex(self.h, bases.h, base_offset, vec.h, offset, n, window_bits, 1, _ptr(out), out_form))
        else:
            self._chk(self.lib.vimz_msm_vec(self.h, bases.h, base_offset, vec.h, offset, n, window_bits, _ptr(out), out_form))
        return out

    def kzg_open(self, srs, vec, z, n=None, offset=0, base_offset=0):
        """vimz_kzg_open: (p(z), proof point) for p(X) = sum_i vec[offset + i] X^i over the SRS powers `srs`; canonical integers."""
        n = vec.n - offset if n is None else n
        lib = self.lib
        lib.vimz_kzg_open.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        ev, pr = np.zeros(4, dtype=np.uint64), np.zeros(8, dtype=np.uint64)
        self._chk(lib.vimz_kzg_open(self.h, srs.h, base_offset, vec.h, offset, n, _ptr(_zlimbs([z], 1)), L.FORM_CANONICAL, _ptr(ev), _ptr(pr)))
        ints = lambda a: sum(int(a[k]) << (64 * k) for k in range(4))
        return ints(ev), (ints(pr[:4]), ints(pr[4:]))

    def mlkzg_open(self, srs, vec, point, n=None, offset=0, seconds=None):
        """vimz_mlkzg_open: (comm as 8 words, eval as an integer, proof as 20·logn + 16 words) of vec[offset : offset + n] read as a multilinear polynomial in
        len(point) variables, over the SRS powers `srs`.  seconds: a dict that receives the four phases."""
        n = vec.n - offset if n is None else n
        lib = self.lib
        lib.vimz_mlkzg_open.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint32] + _MLKZG_TAIL
        return _mlkzg_open(self, lib.vimz_mlkzg_open, (self.h, srs.h, vec.h, offset, n, len(point)), point, seconds)

    # ---- probes
    def field_op(self, field, op, a, b=None):
        a = _u64(a)
        n = a.size // 4
        b = _u64(b) if b is not None else None
        out = np.zeros((n, 4), dtype=np.uint64)
        self._chk(self.lib.vimz_field_op(self.h, field, {"add": 0, "sub": 1, "mul": 2, "inv": 3}[op], _ptr(a), _ptr(b), _ptr(out), n))
        return out

    def curve_add(self, curve, p, q):
        p, q = _u64(p), _u64(q)
        n = p.size // 8
        out = np.zeros((n, 8), dtype=np.uint64)
        self._chk(self.lib.vimz_curve_add(self.h, curve, _ptr(p), _ptr(q), _ptr(out), n))
        return out


class Prover:
    """vimz_prover: GPU folding of one transformation's step circuit (mirrors `fold_input`,
    vimz/src/nova_snark_backend/folding.rs:27-43)."""
    PHASES = ["witness", "state_chain_host", "spmv", "msm_w", "cross_term", "msm_t", "ro_host", "fold", "host_ec"]

    def __init__(self, ctx, circuit, ck, max_batch=16):
        self.ctx, self.circuit, self.ck = ctx, circuit, ck
        lib = ctx.lib
        vp, sz = C.c_void_p, C.c_size_t
        lib.vimz_prover_create.argtypes = [vp, vp, vp, sz, C.POINTER(vp)]
        lib.vimz_prover_free.argtypes = [vp]
        lib.vimz_prover_free.restype = None
        lib.vimz_prover_reset.argtypes = [vp, vp]
        lib.vimz_prover_fold.argtypes = [vp, vp, sz]
        lib.vimz_prover_verify.argtypes = [vp, C.POINTER(C.c_uint32)]
        lib.vimz_prover_instance.argtypes = [vp, vp, vp, vp, vp, C.POINTER(C.c_uint64)]
        lib.vimz_prover_running.argtypes = [vp, vp, vp]
        lib.vimz_prover_profile.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
        lib.vimz_prover_witness.argtypes = [vp, vp, sz, vp, vp, vp]
        lib.vimz_prover_spmv.argtypes = [vp, vp, vp, vp, vp]
        h = vp()
        ctx._chk(lib.vimz_prover_create(ctx.h, circuit.h, ck.h, max_batch, C.byref(h)))
        self.h = h
        self.max_batch = max_batch

    def close(self):
        if self.h:
            self.ctx.lib.vimz_prover_free(self.h)
            self.h = None

    def reset(self, z0):
        z = np.zeros((self.circuit.len_z, 4), dtype=np.uint64)
        for i, v in enumerate(z0):
            for k in range(4):
                z[i, k] = (int(v) >> (64 * k)) & 0xFFFFFFFFFFFFFFFF
        self.ctx._chk(self.ctx.lib.vimz_prover_reset(self.h, _ptr(z)))

    def fold(self, step_inputs):
        """step_inputs: (nsteps, n_priv, 4) uint64 canonical."""
        a = _u64(step_inputs).reshape(-1, self.circuit.n_priv, 4)
        self.ctx._chk(self.ctx.lib.vimz_prover_fold(self.h, _ptr(a), a.shape[0]))

    def fold_witness(self, witnesses):
        """witnesses: (nsteps, n_wires, 4) uint64 canonical, iden3 wire order (e.g. parsed from circom's .wtns files)."""
        a = _u64(witnesses).reshape(-1, self.circuit.n_wires, 4)
        lib = self.ctx.lib
        lib.vimz_prover_fold_witness.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        self.ctx._chk(lib.vimz_prover_fold_witness(self.h, _ptr(a), a.shape[0]))

    def verify(self):
        r = C.c_uint32()
        self.ctx._chk(self.ctx.lib.vimz_prover_verify(self.h, C.byref(r)))
        return r.value

    def instance(self):
        cw, ce, u = np.zeros(8, dtype=np.uint64), np.zeros(8, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
        z = np.zeros((self.circuit.len_z, 4), dtype=np.uint64)
        steps = C.c_uint64()
        self.ctx._chk(self.ctx.lib.vimz_prover_instance(self.h, _ptr(cw), _ptr(ce), _ptr(u), _ptr(z), C.byref(steps)))
        return {"comm_W": cw, "comm_E": ce, "u": u, "z": z, "steps": steps.value}

    def running(self):
        z = np.zeros((self.circuit.n_wires, 4), dtype=np.uint64)
        E = np.zeros((self.circuit.n_constraints, 4), dtype=np.uint64)
        self.ctx._chk(self.ctx.lib.vimz_prover_running(self.h, _ptr(z), _ptr(E)))
        return z, E

    def profile(self):
        s = (C.c_double * 9)()
        n = (C.c_uint64 * 9)()
        self.ctx._chk(self.ctx.lib.vimz_prover_profile(self.h, s, n))
        return {k: {"seconds": s[i], "count": int(n[i])} for i, k in enumerate(self.PHASES)}

    def witness(self, inputs, want_wires=True):
        a = _u64(inputs).reshape(-1, self.circuit.n_priv, 4)
        rows = a.shape[0]
        zw = np.zeros((rows, self.circuit.n_wires, 4), dtype=np.uint64) if want_wires else None
        zs = np.zeros((rows + 1, self.circuit.len_z, 4), dtype=np.uint64)
        st = np.zeros(rows, dtype=np.uint32)
        self.ctx._chk(self.ctx.lib.vimz_prover_witness(self.h, _ptr(a), rows, _ptr(zw), _ptr(zs), _ptr(st)))
        return zw, zs, st

    def spmv(self, z):
        z = _u64(z)
        n = self.circuit.n_constraints
        out = [np.zeros((n, 4), dtype=np.uint64) for _ in range(3)]
        self.ctx._chk(self.ctx.lib.vimz_prover_spmv(self.h, _ptr(z), *[_ptr(o) for o in out]))
        return out

    # ---- multi-GPU support: state chain, export / merge of running instances
    def state_chain(self, z_start, inputs):
        a = _u64(inputs).reshape(-1, self.circuit.n_priv, 4)
        n = a.shape[0]
        z = np.zeros((self.circuit.len_z, 4), dtype=np.uint64)
        for i, v in enumerate(z_start):
            for k in range(4):
                z[i, k] = (int(v) >> (64 * k)) & 0xFFFFFFFFFFFFFFFF
        out = np.zeros((n + 1, self.circuit.len_z, 4), dtype=np.uint64)
        lib = self.ctx.lib
        lib.vimz_prover_state_chain.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        self.ctx._chk(lib.vimz_prover_state_chain(self.h, _ptr(z), _ptr(a), n, _ptr(out)))
        return out

    def export(self):
        lib = self.ctx.lib
        lib.vimz_prover_export_size.argtypes = [C.c_void_p]
        lib.vimz_prover_export_size.restype = C.c_size_t
        lib.vimz_prover_export.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        n = lib.vimz_prover_export_size(self.h)
        buf = np.zeros(n, dtype=np.uint8)
        self.ctx._chk(lib.vimz_prover_export(self.h, _ptr(buf), n))
        return buf

    def merge_prover(self, other):
        """Final fold with another prover on the same GPU (vimz_prover_merge_prover): no host round trip."""
        lib = self.ctx.lib
        lib.vimz_prover_merge_prover.argtypes = [C.c_void_p, C.c_void_p]
        self.ctx._chk(lib.vimz_prover_merge_prover(self.h, other.h))

    def merge(self, blob):
        lib = self.ctx.lib
        lib.vimz_prover_merge.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        self.ctx._chk(lib.vimz_prover_merge(self.h, _ptr(blob), blob.size))


# ---- Nova IVC (include/vimz_hip.h: vimz_ivc_*) --------------------------------------------------------------------------
CX_R1CS = {"A_rowptr": 0, "A_col": 1, "A_coef": 2, "B_rowptr": 3, "B_col": 4, "B_coef": 5, "C_rowptr": 6, "C_col": 7, "C_coef": 8,
           "dict_canon": 10}
IX_RUNNING_Z, IX_RUNNING_E, IX_FRESH_Z, IX_INSTANCE, IX_FRESH_INSTANCE, IX_PARAMS, IX_INFO, IX_LAST_STEP = 100, 101, 102, 103, 104, 105, 106, 107


def _export(fn, *args):
    """Two-call export protocol of the ABI: size query, then copy."""
    n = fn(*args, None, 0)
    if n < 0:
        raise L.VimzError(n, "export")
    buf = np.zeros((n + 7) // 8 + 1, dtype=np.uint64)
    got = fn(*args, _ptr(buf), n)
    if got != n:
        raise L.VimzError(got, "export")
    return buf.view(np.uint8)[:n]


def _r1cs_tables(fn, *args):
    out = {}
    for name, code in CX_R1CS.items():
        a = _export(fn, *args, code)
        out[name] = a.view(np.uint64).reshape(-1, 4) if name == "dict_canon" else a.view(np.uint32)
    return out


class IVC:
    """vimz_ivc: Nova IVC of one transformation's step circuit with the augmented verifier circuits on the BN254/Grumpkin cycle
    (RecursiveSNARK::new / prove_step / verify; reference entry vimz/src/nova_snark_backend/folding.rs:27-56)."""
    PHASES = ["verifier_circuit_primary_host", "verifier_circuit_secondary_host", "wait_secondary_msm", "wait_primary_msm",
              "upload_launch", "producer_wait", "secondary_gpu", "total"]

    def __init__(self, ctx, circuit, ck_primary, ck_secondary, max_batch=16):
        self.ctx, self.circuit = ctx, circuit
        lib = ctx.lib
        vp, sz = C.c_void_p, C.c_size_t
        lib.vimz_ivc_create.argtypes = [vp, vp, vp, vp, sz, C.POINTER(vp)]
        lib.vimz_ivc_free.argtypes = [vp]
        lib.vimz_ivc_free.restype = None
        lib.vimz_ivc_reset.argtypes = [vp, vp]
        lib.vimz_ivc_fold.argtypes = [vp, vp, sz]
        lib.vimz_ivc_fold_witness.argtypes = [vp, vp, sz]
        lib.vimz_ivc_verify.argtypes = [vp, C.c_uint64, vp, C.POINTER(C.c_uint32)]
        lib.vimz_ivc_info.argtypes = [vp, vp]
        lib.vimz_ivc_state.argtypes = [vp, vp, C.POINTER(C.c_uint64)]
        lib.vimz_ivc_profile.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
        lib.vimz_ivc_export.argtypes = [vp, C.c_int, C.c_int, vp, sz]
        lib.vimz_ivc_export.restype = C.c_int64
        h = vp()
        ctx._chk(lib.vimz_ivc_create(ctx.h, circuit.h, ck_primary.h, ck_secondary.h, max_batch, C.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            self.ctx.lib.vimz_ivc_free(self.h)
            self.h = None

    def reset(self, z0):
        z = np.zeros((self.circuit.len_z, 4), dtype=np.uint64)
        for i, v in enumerate(z0):
            for k in range(4):
                z[i, k] = (int(v) >> (64 * k)) & 0xFFFFFFFFFFFFFFFF
        self.ctx._chk(self.ctx.lib.vimz_ivc_reset(self.h, _ptr(z)))

    def add_msm_helper(self, helper_ctx, ck_on_helper):
        """vimz_ivc_add_msm_helper: another GPU (context) takes a base range of every step's large MSM(T)."""
        lib = self.ctx.lib
        lib.vimz_ivc_add_msm_helper.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        self.ctx._chk(lib.vimz_ivc_add_msm_helper(self.h, helper_ctx.h, ck_on_helper.h))

    def fold(self, step_inputs):
        a = _u64(step_inputs).reshape(-1, self.circuit.n_priv, 4)
        self.ctx._chk(self.ctx.lib.vimz_ivc_fold(self.h, _ptr(a), a.shape[0]))

    def fold_witness(self, witnesses):
        a = _u64(witnesses).reshape(-1, self.circuit.n_wires, 4)
        self.ctx._chk(self.ctx.lib.vimz_ivc_fold_witness(self.h, _ptr(a), a.shape[0]))

    def verify(self, num_steps, z0):
        """RecursiveSNARK::verify(pp, num_steps, z0): 0 = accepted (bit 12: not a proof of `num_steps` steps from `z0`)."""
        z = np.zeros((self.circuit.len_z, 4), dtype=np.uint64)
        for i, v in enumerate(z0):
            for k in range(4):
                z[i, k] = (int(v) >> (64 * k)) & 0xFFFFFFFFFFFFFFFF
        r = C.c_uint32()
        self.ctx._chk(self.ctx.lib.vimz_ivc_verify(self.h, int(num_steps), _ptr(z), C.byref(r)))
        return r.value

    def info(self):
        a = np.zeros(12, dtype=np.uint64)
        self.ctx._chk(self.ctx.lib.vimz_ivc_info(self.h, _ptr(a)))
        keys = ["steps", "primary_wires", "primary_constraints", "step_wires", "step_constraints", "secondary_wires", "secondary_constraints",
                "len_z", "verifier_wires", "primary_nnz", "secondary_nnz", "head_rows"]
        return {k: int(a[i]) for i, k in enumerate(keys)}

    def state(self):
        z = np.zeros((self.circuit.len_z, 4), dtype=np.uint64)
        steps = C.c_uint64()
        self.ctx._chk(self.ctx.lib.vimz_ivc_state(self.h, _ptr(z), C.byref(steps)))
        return [sum(int(z[i, k]) << (64 * k) for k in range(4)) for i in range(self.circuit.len_z)], steps.value

    def state_chain(self, z_start, inputs):
        a = _u64(inputs).reshape(-1, self.circuit.n_priv, 4)
        n = a.shape[0]
        z = np.zeros((self.circuit.len_z, 4), dtype=np.uint64)
        for i, v in enumerate(z_start):
            for k in range(4):
                z[i, k] = (int(v) >> (64 * k)) & 0xFFFFFFFFFFFFFFFF
        out = np.zeros((n + 1, self.circuit.len_z, 4), dtype=np.uint64)
        lib = self.ctx.lib
        lib.vimz_ivc_state_chain.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        self.ctx._chk(lib.vimz_ivc_state_chain(self.h, _ptr(z), _ptr(a), n, _ptr(out)))
        return out

    def digest_stride(self):
        """Elements per row of row_digests' output; 0 when this circuit's digests depend on the state (crop)."""
        lib = self.ctx.lib
        lib.vimz_ivc_digest_stride.argtypes = [C.c_void_p]
        lib.vimz_ivc_digest_stride.restype = C.c_size_t
        return int(lib.vimz_ivc_digest_stride(self.h))

    def row_digests(self, inputs):
        """Part (1) of the state chain: the state-independent row hashes of `inputs` ((n, stride, 4) uint64, opaque).  Any GPU can
        compute them for any rows: the ranks of a sharded proof hash their own rows side by side."""
        a = _u64(inputs).reshape(-1, self.circuit.n_priv, 4)
        out = np.zeros((a.shape[0], self.digest_stride(), 4), dtype=np.uint64)
        lib = self.ctx.lib
        lib.vimz_ivc_row_digests.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        self.ctx._chk(lib.vimz_ivc_row_digests(self.h, _ptr(a), a.shape[0], _ptr(out)))
        return out

    def chain_from_digests(self, z_start, inputs, digests):
        """Part (2): the serial chain over rows whose digests are known (host only); returns (n + 1, len_z, 4) states."""
        a = _u64(inputs).reshape(-1, self.circuit.n_priv, 4)
        d = np.ascontiguousarray(digests, dtype=np.uint64).reshape(a.shape[0], -1, 4)
        out = np.zeros((a.shape[0] + 1, self.circuit.len_z, 4), dtype=np.uint64)
        lib = self.ctx.lib
        lib.vimz_ivc_chain_from_digests.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        self.ctx._chk(lib.vimz_ivc_chain_from_digests(self.h, _ptr(_zlimbs(z_start, self.circuit.len_z)), _ptr(a), _ptr(d), a.shape[0], _ptr(out)))
        return out

    def profile(self):
        s = (C.c_double * 8)()
        n = (C.c_uint64 * 8)()
        self.ctx._chk(self.ctx.lib.vimz_ivc_profile(self.h, s, n))
        return {k: (s[i], n[i]) for i, k in enumerate(self.PHASES)}

    def proof_export(self):
        """The proof (and resume state) as bytes: vimz_ivc_proof_export."""
        lib = self.ctx.lib
        lib.vimz_ivc_proof_size.argtypes = [C.c_void_p]
        lib.vimz_ivc_proof_size.restype = C.c_size_t
        lib.vimz_ivc_proof_export.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        n = lib.vimz_ivc_proof_size(self.h)
        buf = np.zeros(n, dtype=np.uint8)
        self.ctx._chk(lib.vimz_ivc_proof_export(self.h, _ptr(buf), n))
        return buf

    def proof_import(self, blob):
        lib = self.ctx.lib
        lib.vimz_ivc_proof_import.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        b = np.ascontiguousarray(blob, dtype=np.uint8)
        self.ctx._chk(lib.vimz_ivc_proof_import(self.h, _ptr(b), b.size))

    def compress(self):
        """CompressedSNARK::prove: returns (proof bytes as uint8 array, {"setup_s", "prove_s"})."""
        lib = self.ctx.lib
        lib.vimz_ivc_compressed_size.argtypes = [C.c_void_p]
        lib.vimz_ivc_compressed_size.restype = C.c_size_t
        lib.vimz_ivc_compress.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_double)]
        n = lib.vimz_ivc_compressed_size(self.h)
        buf = np.zeros(n, dtype=np.uint8)
        sec = (C.c_double * 2)()
        self.ctx._chk(lib.vimz_ivc_compress(self.h, _ptr(buf), n, sec))
        return buf, {"setup_s": sec[0], "prove_s": sec[1]}

    def verify_compressed(self, blob, num_steps, z0):
        """CompressedSNARK::verify(vk, num_steps, z0): 0 = accepted.  This IVC object only supplies the verifier key."""
        lib = self.ctx.lib
        lib.vimz_ivc_verify_compressed.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint32)]
        b = np.ascontiguousarray(blob, dtype=np.uint8)
        z = np.zeros((self.circuit.len_z, 4), dtype=np.uint64)
        for i, v in enumerate(z0):
            for k in range(4):
                z[i, k] = (int(v) >> (64 * k)) & 0xFFFFFFFFFFFFFFFF
        r = C.c_uint32()
        self.ctx._chk(lib.vimz_ivc_verify_compressed(self.h, _ptr(b), b.size, int(num_steps), _ptr(z), C.byref(r)))
        return r.value

    def verify_compressed_batch(self, blobs, num_steps, initial_states, chunk=0, bisect=True, leaf=0, stats=None):
        """vimz_ivc_verify_compressed_batch: many compressed proofs ("ivc" and "merged" kinds, mixed as they come) under this verifier key in one call.
        Returns (words, seconds): words[i] is what verify_compressed / MergedProof.verify_compressed gives for proof i alone.
        bisect, leaf, stats: as verify_decider_batch takes them (a refused chunk is bisected; leaf 0 = 1)."""
        return _compressed_batch(self, "vimz_ivc_verify_compressed_batch", blobs, num_steps, initial_states, chunk, bisect=bisect, leaf=leaf, stats=stats)

    def export(self, side, what):
        """(n, 4) uint64 canonical elements."""
        return _export(self.ctx.lib.vimz_ivc_export, self.h, side, what).view(np.uint64).reshape(-1, 4)

    def r1cs(self, side):
        return _r1cs_tables(self.ctx.lib.vimz_ivc_export, self.h, side)


class CycleFoldIVC:
    """vimz_cf: Nova + CycleFold IVC of one transformation's step circuit (the reference's Sonobe backend: Folding::prove_step / verify,
    vimz/src/sonobe_backend/folding.rs:52-75).  ck_main on BN254 G1 (e.g. a KZG SRS's powers), ck_cyclefold on Grumpkin."""
    PHASES = ["cross_term_msm", "cyclefold_instances", "main_circuit_host", "fresh_instance", "producer_wait", "total", "wait_row_event", "wait_verifier_commitment"]

    def __init__(self, ctx, circuit, ck_main, ck_cyclefold, max_batch=16):
        self.ctx, self.circuit = ctx, circuit
        lib = ctx.lib
        vp, sz = C.c_void_p, C.c_size_t
        lib.vimz_cf_create.argtypes = [vp, vp, vp, vp, sz, C.POINTER(vp)]
        lib.vimz_cf_free.argtypes = [vp]
        lib.vimz_cf_free.restype = None
        lib.vimz_cf_reset.argtypes = [vp, vp]
        lib.vimz_cf_fold.argtypes = [vp, vp, sz]
        lib.vimz_cf_verify.argtypes = [vp, C.c_uint64, vp, C.POINTER(C.c_uint32)]
        lib.vimz_cf_info.argtypes = [vp, vp]
        lib.vimz_cf_state.argtypes = [vp, vp, C.POINTER(C.c_uint64)]
        lib.vimz_cf_profile.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
        lib.vimz_cf_export.argtypes = [vp, C.c_int, C.c_int, vp, sz]
        lib.vimz_cf_export.restype = C.c_int64
        h = vp()
        ctx._chk(lib.vimz_cf_create(ctx.h, circuit.h, ck_main.h, ck_cyclefold.h, max_batch, C.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            self.ctx.lib.vimz_cf_free(self.h)
            self.h = None

    def reset(self, z0):
        self.ctx._chk(self.ctx.lib.vimz_cf_reset(self.h, _ptr(_zlimbs(z0, self.circuit.len_z))))

    def fold(self, step_inputs):
        a = _u64(step_inputs).reshape(-1, self.circuit.n_priv, 4)
        self.ctx._chk(self.ctx.lib.vimz_cf_fold(self.h, _ptr(a), a.shape[0]))

    def verify(self, num_steps, z0):
        r = C.c_uint32()
        self.ctx._chk(self.ctx.lib.vimz_cf_verify(self.h, int(num_steps), _ptr(_zlimbs(z0, self.circuit.len_z)), C.byref(r)))
        return r.value

    def info(self):
        a = np.zeros(12, dtype=np.uint64)
        self.ctx._chk(self.ctx.lib.vimz_cf_info(self.h, _ptr(a)))
        keys = ["steps", "main_wires", "main_constraints", "step_wires", "step_constraints", "cyclefold_wires", "cyclefold_constraints",
                "len_z", "verifier_wires", "main_nnz", "cyclefold_nnz", "cyclefold_io"]
        return {k: int(a[i]) for i, k in enumerate(keys)}

    def state(self):
        z = np.zeros((self.circuit.len_z, 4), dtype=np.uint64)
        steps = C.c_uint64()
        self.ctx._chk(self.ctx.lib.vimz_cf_state(self.h, _ptr(z), C.byref(steps)))
        return [sum(int(z[i, k]) << (64 * k) for k in range(4)) for i in range(self.circuit.len_z)], steps.value

    def profile(self):
        s = (C.c_double * 8)()
        n = (C.c_uint64 * 8)()
        self.ctx._chk(self.ctx.lib.vimz_cf_profile(self.h, s, n))
        return {k: (s[i], n[i]) for i, k in enumerate(self.PHASES)}

    def export(self, side, what):
        return _export(self.ctx.lib.vimz_cf_export, self.h, side, what).view(np.uint64).reshape(-1, 4)

    def r1cs(self, side):
        return _r1cs_tables(self.ctx.lib.vimz_cf_export, self.h, side)

    def compress(self):
        """vimz_cf_compress: the succinct proof of this chain — arguments for U_n, u_n and cfU_n in place of their witnesses.
        Returns (proof bytes as uint8 array, {"setup_s", "prove_s"})."""
        lib = self.ctx.lib
        lib.vimz_cf_compressed_size.argtypes = [C.c_void_p]
        lib.vimz_cf_compressed_size.restype = C.c_size_t
        lib.vimz_cf_compress.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_double)]
        n = lib.vimz_cf_compressed_size(self.h)
        buf = np.zeros(n, dtype=np.uint8)
        sec = (C.c_double * 2)()
        self.ctx._chk(lib.vimz_cf_compress(self.h, _ptr(buf), n, sec))
        return buf, {"setup_s": sec[0], "prove_s": sec[1]}

    def verify_compressed(self, blob, num_steps, z0):
        """vimz_cf_verify_compressed(vk, blob, num_steps, z0): 0 = accepted.  This object only supplies the verifier key."""
        lib = self.ctx.lib
        lib.vimz_cf_verify_compressed.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint32)]
        b = np.ascontiguousarray(blob, dtype=np.uint8)
        r = C.c_uint32()
        self.ctx._chk(lib.vimz_cf_verify_compressed(self.h, _ptr(b), b.size, int(num_steps), _ptr(_zlimbs(z0, self.circuit.len_z)), C.byref(r)))
        return r.value

    def verify_compressed_batch(self, blobs, num_steps, initial_states, chunk=0, bisect=True, leaf=0, stats=None):
        """vimz_cf_verify_compressed_batch: many compressed Nova + CycleFold proofs ("cyclefold" and "cyclefold-merged", mixed) under this verifier key in
        one call.  Returns (words, seconds): words[i] is what the single verifier gives for proof i alone."""
        return _compressed_batch(self, "vimz_cf_verify_compressed_batch", blobs, num_steps, initial_states, chunk, bisect=bisect, leaf=leaf, stats=stats)

    def poke(self, which, index, value):
        """Test hook (vimz_cf_poke, include/vimz_hip_testing.h): exists only when the process runs on libvimz_hip_testing.so
        (VIMZ_HIP_LIBRARY=testing); the product library has no way to overwrite a prover's vectors."""
        lib = self.ctx.lib
        if not hasattr(lib, "vimz_cf_poke"):
            raise L.VimzError(L.ERR_INVALID, "vimz_cf_poke is a test hook: start the process with VIMZ_HIP_LIBRARY=testing")
        lib.vimz_cf_poke.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
        self.ctx._chk(lib.vimz_cf_poke(self.h, which, index, _ptr(_zlimbs([value], 1))))

    def state_chain(self, z_start, inputs):
        a = _u64(inputs).reshape(-1, self.circuit.n_priv, 4)
        out = np.zeros((a.shape[0] + 1, self.circuit.len_z, 4), dtype=np.uint64)
        lib = self.ctx.lib
        lib.vimz_cf_state_chain.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        self.ctx._chk(lib.vimz_cf_state_chain(self.h, _ptr(_zlimbs(z_start, self.circuit.len_z)), _ptr(a), a.shape[0], _ptr(out)))
        return out

    def kzg_open(self, which, z):
        """vimz_cf_kzg_open: (eval, proof point) of the running main instance's comm_W (which = 0) or comm_E (1) at z."""
        lib = self.ctx.lib
        lib.vimz_cf_kzg_open.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        ev, pr = np.zeros(4, dtype=np.uint64), np.zeros(8, dtype=np.uint64)
        self.ctx._chk(lib.vimz_cf_kzg_open(self.h, which, _ptr(_zlimbs([z], 1)), _ptr(ev), _ptr(pr)))
        ints = lambda a: sum(int(a[k]) << (64 * k) for k in range(4))
        return ints(ev), (ints(pr[:4]), ints(pr[4:]))

    def mlkzg_open(self, which, point, seconds=None):
        """vimz_cf_mlkzg_open: (comm, eval, proof) as Context.mlkzg_open gives them for the running main instance's comm_W (which = 0) or comm_E (1); len(point) must
        be the least logn with 2^logn >= the vector's length."""
        lib = self.ctx.lib
        lib.vimz_cf_mlkzg_open.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32] + _MLKZG_TAIL[1:]
        return _mlkzg_open(self.ctx, lib.vimz_cf_mlkzg_open, (self.h, which), point, seconds, point_first=True)

    def digest_stride(self):
        lib = self.ctx.lib
        lib.vimz_cf_digest_stride.argtypes = [C.c_void_p]
        lib.vimz_cf_digest_stride.restype = C.c_size_t
        return int(lib.vimz_cf_digest_stride(self.h))

    def row_digests(self, inputs):
        a = _u64(inputs).reshape(-1, self.circuit.n_priv, 4)
        out = np.zeros((a.shape[0], self.digest_stride(), 4), dtype=np.uint64)
        lib = self.ctx.lib
        lib.vimz_cf_row_digests.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        self.ctx._chk(lib.vimz_cf_row_digests(self.h, _ptr(a), a.shape[0], _ptr(out)))
        return out

    def chain_from_digests(self, z_start, inputs, digests):
        a = _u64(inputs).reshape(-1, self.circuit.n_priv, 4)
        d = np.ascontiguousarray(digests, dtype=np.uint64).reshape(a.shape[0], -1, 4)
        out = np.zeros((a.shape[0] + 1, self.circuit.len_z, 4), dtype=np.uint64)
        lib = self.ctx.lib
        lib.vimz_cf_chain_from_digests.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        self.ctx._chk(lib.vimz_cf_chain_from_digests(self.h, _ptr(_zlimbs(z_start, self.circuit.len_z)), _ptr(a), _ptr(d), a.shape[0], _ptr(out)))
        return out

    def proof_export(self):
        """The proof (and resume state) as bytes: vimz_cf_proof_export."""
        lib = self.ctx.lib
        lib.vimz_cf_proof_size.argtypes = [C.c_void_p]
        lib.vimz_cf_proof_size.restype = C.c_size_t
        lib.vimz_cf_proof_export.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        n = lib.vimz_cf_proof_size(self.h)
        buf = np.zeros(n, dtype=np.uint8)
        self.ctx._chk(lib.vimz_cf_proof_export(self.h, _ptr(buf), n))
        return buf

    def proof_import(self, blob):
        lib = self.ctx.lib
        lib.vimz_cf_proof_import.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        b = np.ascontiguousarray(blob, dtype=np.uint8)
        self.ctx._chk(lib.vimz_cf_proof_import(self.h, _ptr(b), b.size))


def cyclefold_selfcheck_last_step(steps=4):
    """vimz_cf_selfcheck_last_step (host only): (digest, z_0, uint64 words of the last step's VIMZ_IX_LAST_STEP record)."""
    from . import _lib
    lib = _lib.testing_lib()
    lib.vimz_cf_selfcheck_last_step.argtypes = [C.c_int, C.c_void_p, C.c_size_t]
    lib.vimz_cf_selfcheck_last_step.restype = C.c_int64
    n = lib.vimz_cf_selfcheck_last_step(int(steps), None, 0)
    if n < 0:
        raise _lib.VimzError(int(n), "vimz_cf_selfcheck_last_step")
    buf = np.zeros(n // 8, dtype=np.uint64)
    assert lib.vimz_cf_selfcheck_last_step(int(steps), _ptr(buf), n) == n
    ints = lambda a: sum(int(a[k]) << (64 * k) for k in range(4))
    return ints(buf[0:4]), ints(buf[4:8]), buf[8:]


def cyclefold_selfcheck_merge(segs_run0=3, segs_run1=2):
    """vimz_cf_selfcheck_merge (host only): (digest, record words, accumulator dict) of made-up segment records replayed by the library."""
    from . import _lib
    lib = _lib.testing_lib()
    lib.vimz_cf_selfcheck_merge.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    lib.vimz_cf_selfcheck_merge.restype = C.c_int64
    n = lib.vimz_cf_selfcheck_merge(segs_run0, segs_run1, None, 0)
    if n < 0:
        raise _lib.VimzError(int(n), "vimz_cf_selfcheck_merge")
    buf = np.zeros(n // 8, dtype=np.uint64)
    assert lib.vimz_cf_selfcheck_merge(segs_run0, segs_run1, _ptr(buf), n) == n
    w = [int(x) for x in buf]
    el = lambda pos: sum(w[pos + k] << (64 * k) for k in range(4))
    dg, nrec = el(0), w[4]
    rec = buf[5:5 + nrec]
    pos = 5 + nrec
    acc = {"n": w[pos], "zs": [el(pos + 1)], "ze": [el(pos + 5)]}
    pos += 9
    vals = [el(pos + 4 * k) for k in range(7 + 12)]
    acc["P"] = [(vals[0], vals[1]), (vals[2], vals[3]), vals[4], vals[5], vals[6]]
    acc["Q"] = [(vals[7], vals[8]), (vals[9], vals[10]), vals[11], vals[12:19]]
    return dg, rec, acc


def kzg_setup(ctx, n, seed=None):
    """KZG::setup: (srs as Bases — use it as ck_main of a CycleFoldIVC —, vk_g2 = [tau]G2 as a (4, 4) uint64 array for Decider).  tau comes from the
    OS's randomness and is forgotten; `seed` (bytes) selects the deterministic TEST setup of libvimz_hip_testing.so instead."""
    vp = C.c_void_p
    h = vp()
    vk = np.zeros((4, 4), dtype=np.uint64)
    if seed is None:
        ctx.lib.vimz_kzg_setup.argtypes = [vp, C.c_size_t, C.POINTER(vp), vp]
        ctx._chk(ctx.lib.vimz_kzg_setup(ctx.h, n, C.byref(h), _ptr(vk)))
    else:
        fn = _seeded(ctx, "vimz_testing_kzg_setup_seeded")
        fn.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_size_t, C.POINTER(vp), vp]
        ctx._chk(fn(ctx.h, bytes(seed), len(seed), n, C.byref(h), _ptr(vk)))
    return Bases(ctx, h, L.CURVE_BN254_G1, n), vk


_BN254_Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583


POWERS_PROBLEMS = {0x1: "a coordinate is not below q", 0x2: "a point is not on its curve", 0x4: "a point is the identity", 0x8: "a point of G2 is outside the subgroup",
                   0x10: "a first point is not the generator", 0x20: "tau_g1 is not the powers of one tau", 0x40: "alpha_g1 is not the powers of one tau",
                   0x80: "beta_g1 is not the powers of one tau", 0x100: "tau_g2 is not the powers of one tau", 0x200: "tau_g1[1] and tau_g2[1] are not of one tau",
                   0x400: "beta_g1[0] and beta_g2 are not of one beta"}      # VIMZ_POWERS_*
POWERS_ARRAYS = (None, "tau_g1", "tau_g2", "alpha_g1", "beta_g1", "beta_g2")      # first_bad[0]


def verify_powers(ctx, powers, n=None, seconds=None, n_tau_g1=None):
    """vimz_powers_verify: judges a powers-of-tau string (iden3.read_ptau's dictionary, the file's Montgomery form) on the GPU — what snarkjs's `powersoftau verify`
    does: every point on its curve and not the identity, every point of G2 in the subgroup, each array the powers of ONE tau (random combinations of 128-bit
    scalars and six pairing equations), the halves of one tau, beta_g1 and beta_g2 of one beta, the first points the generators.  n: the points of tau_g2, alpha_g1
    and beta_g1 to judge, tau_g1 then 2n − 1 (or n_tau_g1) — the prefix a set-up over a domain of n reads; None: the whole string.  Returns (result, first_bad):
    result 0 = accepted, otherwise a union of POWERS_PROBLEMS' bits; first_bad = (array number — POWERS_ARRAYS names it —, index) of the first per-point
    finding, (0, 0) when there is none.  seconds: a list that receives [host conversion, per-point flags, combinations, pairings].  VimzError(ERR_INVALID): n
    below 2 or beyond the string."""
    a = {name: np.ascontiguousarray(powers[name], dtype=np.uint64).reshape(-1, 8 * group) for name, group in _LAGRANGE_ARRAYS + (("beta_g2", 2),)}
    have = min(a["tau_g2"].shape[0], a["alpha_g1"].shape[0], a["beta_g1"].shape[0])
    n_pow = have if n is None else int(n)
    n_g1 = int(n_tau_g1) if n_tau_g1 is not None else a["tau_g1"].shape[0] if n is None else 2 * n_pow - 1
    if n_pow < 2 or n_pow > have or n_g1 < n_pow or n_g1 > a["tau_g1"].shape[0] or a["beta_g2"].shape[0] < 1:
        raise L.VimzError(L.ERR_INVALID, f"verify_powers: {n_pow} points (tau_g1: {n_g1}) of a string that holds {have} (tau_g1: {a['tau_g1'].shape[0]}); needs 2 <= n <= the string's length")
    vp = C.c_void_p
    result, first, sec = C.c_uint32(0), np.zeros(2, dtype=np.uint64), (C.c_double * 4)()
    ctx.lib.vimz_powers_verify.argtypes = [vp, vp, C.c_size_t, vp, vp, vp, C.c_size_t, vp, C.c_int, C.POINTER(C.c_uint32), vp, C.POINTER(C.c_double)]
    ctx._chk(ctx.lib.vimz_powers_verify(ctx.h, _ptr(a["tau_g1"]), n_g1, _ptr(a["tau_g2"]), _ptr(a["alpha_g1"]), _ptr(a["beta_g1"]), n_pow, _ptr(a["beta_g2"]), L.FORM_MONTGOMERY,
                                        C.byref(result), _ptr(first), sec))
    if seconds is not None:
        seconds[:] = list(sec)
    return int(result.value), (int(first[0]), int(first[1]))


def powers_problems(result):
    """the names of a verdict's bits"""
    return [name for bit, name in POWERS_PROBLEMS.items() if result & bit]


def require_good_powers(ctx, powers, n, who, n_tau_g1=None):
    """verify_powers over the prefix a set-up reads; VimzError(ERR_INVALID) naming the problems and first_bad unless the string is accepted"""
    result, first = verify_powers(ctx, powers, n, n_tau_g1=n_tau_g1)
    if result:
        at = f" (first: {POWERS_ARRAYS[first[0]]}[{first[1]}])" if first[0] else ""
        raise L.VimzError(L.ERR_INVALID, f"{who}: the powers-of-tau string is refused: " + "; ".join(powers_problems(result)) + at)


def kzg_from_powers(ctx, powers, n, verify_powers=False):
    """KZG's keys from a powers-of-tau string (iden3.read_ptau's dictionary: rows of uint64 words in the file's Montgomery form) instead of kzg_setup: the srs is
    the string's first n points [tau^k]G1 as Bases, vk_g2 = [tau]G2 = tau_g2[1] as the canonical (4, 4) array Decider takes — no tau is drawn in this process, and
    a decider key derived from the same string shares its tau (as snarkjs's set-ups over one `.ptau` do).  VimzError(ERR_INVALID): n below 2 (the decider checks
    e(srs[1], G2) = e(G1, vk)), a string shorter than n, a first power that is not the generator, a coordinate of tau_g2[1] not below q.  The points are not
    judged otherwise unless verify_powers is true: the string's first n points (tau_g1: 2n − 1, or as many as it holds) then go through vimz_powers_verify first
    (hip.verify_powers: subgroup membership and the same-ratio check of every power) and a refused string raises VimzError(ERR_INVALID) naming the problems.
    That check is opt-in; the pairing check of srs[1] against the key is the decider's."""
    g1 = np.ascontiguousarray(powers["tau_g1"], dtype=np.uint64).reshape(-1, 8)
    g2 = np.ascontiguousarray(powers["tau_g2"], dtype=np.uint64).reshape(-1, 16)
    n = int(n)
    if n < 2 or n > g1.shape[0] or g2.shape[0] < 2:
        raise L.VimzError(L.ERR_INVALID, f"kzg_from_powers: n = {n} with {g1.shape[0]} powers in G1 and {g2.shape[0]} in G2 (needs 2 <= n <= the string's length)")
    ints = lambda row: [int.from_bytes(row[4 * i:4 * i + 4].tobytes(), "little") for i in range(row.size // 4)]      # noqa: E731
    mont = 1 << 256
    if ints(g1[0]) != [mont % _BN254_Q, 2 * mont % _BN254_Q]:
        raise L.VimzError(L.ERR_INVALID, "kzg_from_powers: tau_g1[0] is not the generator of G1")
    vk = ints(g2[1])
    if max(vk) >= _BN254_Q:
        raise L.VimzError(L.ERR_INVALID, "kzg_from_powers: a coordinate of tau_g2[1] is not below the modulus")
    if verify_powers:
        have = min(np.asarray(powers[name]).reshape(-1, 8 * group).shape[0] for name, group in _LAGRANGE_ARRAYS[1:])      # (tau_g1 is about twice as long as the others)
        require_good_powers(ctx, powers, min(n, have), "kzg_from_powers", n_tau_g1=min(2 * n - 1, g1.shape[0]))
    minv = pow(mont, -1, _BN254_Q)
    vk_words = np.frombuffer(b"".join((c * minv % _BN254_Q).to_bytes(32, "little") for c in vk), dtype="<u8").reshape(4, 4).astype(np.uint64)
    return ctx.bases_upload(L.CURVE_BN254_G1, g1[:n], form=L.FORM_MONTGOMERY), vk_words


_LAGRANGE_ARRAYS = (("tau_g1", 1), ("alpha_g1", 1), ("beta_g1", 1), ("tau_g2", 2))      # name, group

POWCHAIN_BITS = {0x1: "a coordinate is not below q", 0x2: "a point is not on its curve", 0x4: "a point is the identity", 0x8: "a record's proof of knowledge of tau' fails",
                 0x10: "a record's proof of knowledge of alpha' fails", 0x20: "a record's proof of knowledge of beta' fails",
                 0x40: "the last record's points are not the final string's", 0x80: "the final string is refused"}      # VIMZ_POWCHAIN_*
POWCHAIN_BIT_NAMES = ("COORD", "OFF_CURVE", "IDENTITY", "KNOWLEDGE_TAU", "KNOWLEDGE_ALPHA", "KNOWLEDGE_BETA", "LAST", "STRING")
POWCHAIN_PLACES = (None, "the origin's point", "record", "the final string's tau_g1 point", "the final string's tau_g2 point", "the final string's alpha_g1 point",
                   "the final string's beta_g1 point", "the final string's beta_g2 point")      # first_bad[0]: VIMZ_POWCHAIN_AT_*
POWCHAIN_RECORD_BYTES = 488
_POWERS_ARRAYS = _LAGRANGE_ARRAYS + (("beta_g2", 2),)


def _powers_args(powers, who):
    """the five arrays of a string as contiguous uint64 rows, and (n_tau_g1, n_pow)"""
    a = {name: np.ascontiguousarray(powers[name], dtype=np.uint64).reshape(-1, 8 * group) for name, group in _POWERS_ARRAYS}
    n_pow = a["tau_g2"].shape[0]
    if n_pow < 2 or a["alpha_g1"].shape[0] != n_pow or a["beta_g1"].shape[0] != n_pow or a["tau_g1"].shape[0] < n_pow or a["beta_g2"].shape[0] != 1:
        raise L.VimzError(L.ERR_INVALID, f"{who}: a string holds n >= 2 points each of tau_g2, alpha_g1 and beta_g1, n or more of tau_g1 and one of beta_g2")
    return a, a["tau_g1"].shape[0], n_pow


def contribute_powers(ctx, powers, secrets=None, nonces=None, seconds=None):
    """vimz_powers_contribute: one contribution to a powers-of-tau string (iden3.read_ptau's dictionary, the file's Montgomery form; what snarkjs's `powersoftau
    contribute` does) — tau', alpha', beta' drawn from the OS and forgotten, every point multiplied by its own scalar on the GPU: the string of (tau, alpha, beta)
    becomes the string of (tau·tau', alpha·alpha', beta·beta').  Returns (powers, record): a dictionary in read_ptau's form (iden3.write_ptau takes it) and the
    record's POWCHAIN_RECORD_BYTES bytes (this project's own format: include/vimz_hip.h) — keep the records of a chain one after another, verify_powers_contributions
    takes them.  secrets and nonces (three ints each, both or neither) select the TEST hook of libvimz_hip_testing.so.  seconds: a list that receives [host, device,
    total].  VimzError(ERR_INVALID): a coordinate not below q, a point off its curve, tau_g1[1], alpha_g1[0] or beta_g1[0] the identity."""
    a, n_g1, n_pow = _powers_args(powers, "contribute_powers")
    out = {name: np.zeros_like(arr) for name, arr in a.items()}
    rec, sec = np.zeros(61, dtype=np.uint64), (C.c_double * 3)()
    vp = C.c_void_p
    if (secrets is None) != (nonces is None):
        raise L.VimzError(L.ERR_INVALID, "contribute_powers: secrets= and nonces= go together")
    argtypes = [vp, vp, C.c_size_t, vp, vp, vp, C.c_size_t, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    if secrets is None:
        fn, extra = ctx.lib.vimz_powers_contribute, ()
    else:
        fn = _seeded(ctx, "vimz_testing_powers_contribute_secrets")
        words = [np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in three), dtype="<u8").astype(np.uint64) for three in (secrets, nonces)]
        if words[0].size != 12 or words[1].size != 12:
            raise L.VimzError(L.ERR_INVALID, "contribute_powers: three secrets and three nonces")
        extra, argtypes = (_ptr(words[0]), _ptr(words[1])), argtypes + [vp, vp]
    fn.argtypes = argtypes + [C.POINTER(C.c_double)]
    ctx._chk(fn(ctx.h, _ptr(a["tau_g1"]), n_g1, _ptr(a["tau_g2"]), _ptr(a["alpha_g1"]), _ptr(a["beta_g1"]), n_pow, _ptr(a["beta_g2"]), L.FORM_MONTGOMERY,
                _ptr(out["tau_g1"]), _ptr(out["tau_g2"]), _ptr(out["alpha_g1"]), _ptr(out["beta_g1"]), _ptr(out["beta_g2"]), _ptr(rec), *extra, sec))
    if seconds is not None:
        seconds[:] = list(sec)
    for key in ("power", "ceremony_power"):
        if key in powers:
            out[key] = int(powers[key])
    return out, rec.tobytes()


def powers_origin_points(origin):
    """the 24 canonical words vimz_powers_verify_contributions takes for a chain's origin: from a string (read_ptau's dictionary: its tau_g1[1], alpha_g1[0],
    beta_g1[0] out of the Montgomery form), from three (x, y) pairs of ints, or 24 words as they are"""
    if isinstance(origin, dict):
        rows = [np.ascontiguousarray(origin["tau_g1"], dtype=np.uint64).reshape(-1, 8)[1], np.ascontiguousarray(origin["alpha_g1"], dtype=np.uint64).reshape(-1, 8)[0],
                np.ascontiguousarray(origin["beta_g1"], dtype=np.uint64).reshape(-1, 8)[0]]
        raw, minv = b"".join(r.astype("<u8").tobytes() for r in rows), pow(1 << 256, -1, _BN254_Q)
        coords = [int.from_bytes(raw[i:i + 32], "little") for i in range(0, 192, 32)]
        if max(coords) >= _BN254_Q:
            raise L.VimzError(L.ERR_INVALID, "verify_powers_contributions: a coordinate of the origin's points is not below q")
        coords = [c * minv % _BN254_Q for c in coords]
    elif isinstance(origin, np.ndarray):
        return np.ascontiguousarray(origin, dtype=np.uint64).reshape(24)
    else:
        coords = [int(c) for p in origin for c in p]
        if len(coords) != 6 or min(coords) < 0 or max(coords) >= 1 << 256:
            raise L.VimzError(L.ERR_INVALID, "verify_powers_contributions: the origin is a string, 24 words or three (x, y) points")
    return np.frombuffer(b"".join(c.to_bytes(32, "little") for c in coords), dtype="<u8").astype(np.uint64)


def verify_powers_contributions(ctx, origin, final, records, seconds=None):
    """vimz_powers_verify_contributions: is `final` (a string in read_ptau's form) what the contributions of `records` (bytes, POWCHAIN_RECORD_BYTES each, in order;
    may be empty) made of `origin` — a string, or its three points tau_g1[1], alpha_g1[0], beta_g1[0] (powers_origin_points)?  Returns (bits, string_bits, first_bad):
    bits 0 = accepted, otherwise a union of POWCHAIN_BITS; string_bits: verify_powers' verdict on the final string when that is what refuses (POWERS_PROBLEMS);
    first_bad = (place — POWCHAIN_PLACES names it —, index).  An accepted chain means the final string is the powers of one tau with consistent alpha and beta that
    nobody knows if any ONE contributor forgot their secrets, whatever the origin was; there is no random beacon and no compatibility with snarkjs's transcript.
    seconds: a list that receives [points, knowledge, the string's verdict]."""
    a, n_g1, n_pow = _powers_args(final, "verify_powers_contributions")
    o = powers_origin_points(origin)
    r = np.ascontiguousarray(np.frombuffer(bytes(records), dtype=np.uint8) if isinstance(records, (bytes, bytearray, memoryview)) else records, dtype=np.uint8).reshape(-1)
    if r.size % POWCHAIN_RECORD_BYTES:
        raise L.VimzError(L.ERR_INVALID, f"verify_powers_contributions: records are {POWCHAIN_RECORD_BYTES} bytes each, not {r.size} in all")
    vp = C.c_void_p
    result, sresult, first, sec = C.c_uint32(0), C.c_uint32(0), np.zeros(2, dtype=np.uint64), (C.c_double * 3)()
    fn = ctx.lib.vimz_powers_verify_contributions
    fn.argtypes = [vp, vp, vp, C.c_size_t, vp, vp, vp, C.c_size_t, vp, C.c_int, vp, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), vp, C.POINTER(C.c_double)]
    ctx._chk(fn(ctx.h, _ptr(o), _ptr(a["tau_g1"]), n_g1, _ptr(a["tau_g2"]), _ptr(a["alpha_g1"]), _ptr(a["beta_g1"]), n_pow, _ptr(a["beta_g2"]), L.FORM_MONTGOMERY,
                _ptr(r) if r.size else None, r.size // POWCHAIN_RECORD_BYTES, C.byref(result), C.byref(sresult), _ptr(first), sec))
    if seconds is not None:
        seconds[:] = list(sec)
    return int(result.value), int(sresult.value), (int(first[0]), int(first[1]))


def powchain_problems(bits):
    """the names of a powers chain verdict's bits"""
    return [name for bit, name in POWCHAIN_BITS.items() if bits & bit]


def powers_lagrange(ctx, group, points, logn, form=L.FORM_CANONICAL, seconds=None):
    """vimz_powers_lagrange: the first 2^logn of `points` (rows of 8 words for group 1 = G1, of 16 for group 2 = G2) -> the points [L_j] in the same form, the
    inverse transform over points on the GPU.  seconds: a list that receives [host conversion and checks, device]."""
    pts = _u64(points).reshape(-1, 8 * group)
    out = np.zeros((1 << logn, 8 * group), dtype=np.uint64)
    sec = (C.c_double * 2)()
    ctx.lib.vimz_powers_lagrange.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_double)]
    ctx._chk(ctx.lib.vimz_powers_lagrange(ctx.h, group, _ptr(pts), pts.shape[0], form, logn, _ptr(out), sec))
    if seconds is not None:
        seconds[:] = list(sec)
    return out


def lagrange_from_powers(ctx, powers, logn):
    """The Lagrange bases of a powers-of-tau string (iden3.read_ptau's dictionary: rows of uint64 words in the file's Montgomery form) over the domain of
    n = 2^logn points: {"tau_g1", "alpha_g1", "beta_g1": (n, 8), "tau_g2": (n, 16)} in the same form, row j = [L_j(tau)]G1, [alpha·L_j(tau)]G1, [beta·L_j(tau)]G1,
    [L_j(tau)]G2 — what snarkjs's `powersoftau prepare phase2` derives, by four calls of vimz_powers_lagrange (the inverse transform over points, on the GPU).
    With them a commitment to a polynomial given by its evaluations e is ctx.msm over the tau_g1 rows and e.  VimzError(ERR_INVALID), before any GPU work: logn
    below 1 or above the string's power, an array shorter than n; from the library: a coordinate not below q, a point not on its curve.  Subgroup membership
    in G2 and the same-ratio property of the string are judged by hip.verify_powers (vimz_powers_verify), which is opt-in: this call does not run it (DESIGN.md §8
    item 5)."""
    logn = int(logn)
    if logn < 1 or logn > int(powers["power"]):
        raise L.VimzError(L.ERR_INVALID, f"lagrange_from_powers: logn = {logn} with a string of power {int(powers['power'])} (needs 1 <= logn <= the power)")
    n = 1 << logn
    arrays = {}
    for name, group in _LAGRANGE_ARRAYS:
        a = np.ascontiguousarray(powers[name], dtype=np.uint64).reshape(-1, 8 * group)
        if a.shape[0] < n:
            raise L.VimzError(L.ERR_INVALID, f"lagrange_from_powers: {name} holds {a.shape[0]} points, the domain has {n}")
        arrays[name] = a[:n]
    return {name: powers_lagrange(ctx, group, arrays[name], logn, form=L.FORM_MONTGOMERY) for name, group in _LAGRANGE_ARRAYS}


def _seeded(ctx, name):
    if not hasattr(ctx.lib, name):
        raise RuntimeError(f"{name} exists only in libvimz_hip_testing.so (start the process with VIMZ_HIP_LIBRARY=testing): seeded setups are test hooks")
    return getattr(ctx.lib, name)


KEYCHAIN_BITS = {0x1: "a coordinate is not below q", 0x2: "a point is not on its curve", 0x4: "a delta point is the identity, or a point of l‖h is in one key only",
                 0x8: "a delta2 is outside the subgroup", 0x10: "the keys differ outside delta1, delta2, l and h", 0x20: "a record's delta1 and delta2 are not of one delta",
                 0x40: "a record's proof of knowledge fails", 0x80: "the last record's delta points are not the final key's",
                 0x100: "l‖h of the final key is not l‖h of the origin over the ratio of their delta2"}      # VIMZ_KEYCHAIN_*
KEYCHAIN_PLACES = (None, "the origin key's delta point", "the final key's delta point", "record", "the origin key's l‖h point", "the final key's l‖h point",
                   "word of the fixed part")      # first_bad[0]: VIMZ_KEYCHAIN_AT_*
KEYCHAIN_RECORD_BYTES = 296


def contribute_key(ctx, blob, delta=None, nonce=None, seconds=None):
    """vimz_decider_key_contribute: a further delta contribution to a saved key (Decider.save_key's bytes; phase 2 of a Groth16 ceremony) — delta1, delta2 times a
    delta' drawn from the OS and forgotten, the l and h queries times 1/delta' on the GPU, every other byte copied.  Needs a context, no prover: the layout is read
    from the blob's header.  Returns (key bytes, record): uint8 arrays, the record KEYCHAIN_RECORD_BYTES long (this project's own format: include/vimz_hip.h) — keep
    the records of a chain one after another, verify_key_contributions takes them.  delta and nonce (ints, both or neither) select the TEST hook of
    libvimz_hip_testing.so.  seconds: a list that receives [host, device, total].  VimzError(ERR_INVALID): not a key, a coordinate not below q, a bad delta point.
    A packed key (pack_key's bytes) is unpacked on the context first, and the key comes back packed: the form it was given."""
    blob, was_packed = _plain_key(ctx, blob)
    b = np.ascontiguousarray(np.frombuffer(bytes(blob), dtype=np.uint8) if isinstance(blob, (bytes, bytearray, memoryview)) else blob, dtype=np.uint8)
    out, rec, sec = np.zeros(b.size, dtype=np.uint8), np.zeros(37, dtype=np.uint64), (C.c_double * 3)()
    vp = C.c_void_p
    if (delta is None) != (nonce is None):
        raise L.VimzError(L.ERR_INVALID, "contribute_key: delta= and nonce= go together")
    if delta is None:
        fn = ctx.lib.vimz_decider_key_contribute
        fn.argtypes, args = [vp, vp, C.c_size_t, vp, C.c_size_t, vp, C.POINTER(C.c_double)], (sec,)
    else:
        fn = _seeded(ctx, "vimz_testing_decider_key_contribute_delta")
        fn.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, vp, vp, vp, C.POINTER(C.c_double)]
        words = [np.frombuffer(int(x).to_bytes(32, "little"), dtype="<u8").astype(np.uint64) for x in (delta, nonce)]
        args = (_ptr(words[0]), _ptr(words[1]), sec)
    fn.restype = C.c_int64
    got = fn(ctx.h, _ptr(b), b.size, _ptr(out), out.size, _ptr(rec), *args)
    if got != b.size:
        ctx._chk(int(got) if got < 0 else L.ERR_INVALID)
    if seconds is not None:
        seconds[:] = list(sec)
    return (pack_key(ctx, out) if was_packed else out), rec.view(np.uint8)


def verify_key_contributions(ctx, origin, final, records, seconds=None):
    """vimz_decider_key_verify_contributions: is `final` the key `origin` after the contributions of `records` (bytes, KEYCHAIN_RECORD_BYTES each, in order; may be
    empty)?  Returns (bits, first_bad): bits 0 = accepted, otherwise a union of KEYCHAIN_BITS; first_bad = (place — KEYCHAIN_PLACES names it —, index).  A verified
    chain means the final key is sound if the origin is and any ONE contributor forgot their delta'.  seconds: a list that receives [host conversion and point checks,
    per-point flags, combination, equations].  VimzError(ERR_INVALID): a key or a record with the wrong magic or length.  Either key may be packed (pack_key's bytes):
    it is unpacked on the context first."""
    origin, final = _plain_key(ctx, origin)[0], _plain_key(ctx, final)[0]
    as_u8 = lambda x: np.ascontiguousarray(np.frombuffer(bytes(x), dtype=np.uint8) if isinstance(x, (bytes, bytearray, memoryview)) else x, dtype=np.uint8).reshape(-1)      # noqa: E731
    o, f, r = as_u8(origin), as_u8(final), as_u8(records)
    if r.size % KEYCHAIN_RECORD_BYTES:
        raise L.VimzError(L.ERR_INVALID, f"verify_key_contributions: records are {KEYCHAIN_RECORD_BYTES} bytes each, not {r.size} in all")
    vp = C.c_void_p
    result, first, sec = C.c_uint32(0), np.zeros(2, dtype=np.uint64), (C.c_double * 4)()
    fn = ctx.lib.vimz_decider_key_verify_contributions
    fn.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_uint32), vp, C.POINTER(C.c_double)]
    ctx._chk(fn(ctx.h, _ptr(o), o.size, _ptr(f), f.size, _ptr(r) if r.size else None, r.size // KEYCHAIN_RECORD_BYTES, C.byref(result), _ptr(first), sec))
    if seconds is not None:
        seconds[:] = list(sec)
    return int(result.value), (int(first[0]), int(first[1]))


def keychain_problems(bits):
    """the names of a chain verdict's bits"""
    return [name for bit, name in KEYCHAIN_BITS.items() if bits & bit]


KEYORIGIN_BITS = {0x1: "a coordinate is not below q", 0x2: "a point is not on its curve", 0x4: "a delta point is the identity, or delta1 and delta2 are not of one delta",
                  0x8: "delta2 or a point of b2 is outside the subgroup", 0x10: "the header (sizes, mode, pp_hash) is not this prover's decider circuit's",
                  0x20: "alpha1, beta1, beta2, gamma2 or the KZG point is not the string's", 0x40: "the a query is not the string's and circuit's",
                  0x80: "the b1 query is not the string's and circuit's", 0x100: "the b2 query is not the string's and circuit's", 0x200: "the ic points are not the string's and circuit's",
                  0x400: "the l query is not the string's and circuit's over delta2", 0x800: "the h query is not the string's over delta2"}      # VIMZ_KEYORIGIN_*
KEYORIGIN_BIT_NAMES = ("COORD", "OFF_CURVE", "DELTA", "SUBGROUP", "HEADER", "FIXED_POINTS", "A", "B1", "B2", "IC", "L", "H")
KEYORIGIN_PLACES = (None, "header word", "fixed word (0 KZG, 1 alpha1, 2 beta1, 3 beta2, 4 gamma2)", "delta point", "ic point", "a point", "b1 point", "l point", "h point",
                    "b2 point")      # first_bad[0]: VIMZ_KEYORIGIN_AT_*


def verify_key_origin(prover, powers, blob, verify_powers=False, seconds=None):
    """vimz_decider_key_verify_origin: is `blob` (Decider.save_key's bytes, from anyone) the key a set-up from `powers` (iden3.read_ptau's dictionary) derives for
    `prover`'s decider circuit — light or full as the blob says —, for the delta its delta points commit to?  What snarkjs's `zkey verify` checks against an r1cs and a
    ptau; delta is never known and nothing is derived again (random combinations under 128-bit scalars from the OS: sparse products of the circuit's matrices, inverse
    NTTs and MSMs over the string on the GPU, three products of pairings).  Returns (result, first_bad): result 0 = accepted, otherwise a union of KEYORIGIN_BITS;
    first_bad = (place — KEYORIGIN_PLACES names it —, index), (0, 0) when only equations fail.  A key that has had contributions passes too; who contributed is
    verify_key_contributions' matter.  The string is taken as given unless verify_powers is true: the prefix the key's domain reads then goes through hip.verify_powers
    first and a refused string raises VimzError(ERR_INVALID) before any key work.  seconds: a list that receives [circuit synthesis, host conversion + fixed words,
    per-point flags, circuit side, key-side combinations + pairings].  VimzError(ERR_INVALID): not a key, a string shorter than the key's domain needs, a bad point of
    the string.  A packed key (pack_key's bytes) is unpacked on the prover's context first."""
    ctx = prover.ctx
    blob = _plain_key(ctx, blob)[0]
    b = np.ascontiguousarray(np.frombuffer(bytes(blob), dtype=np.uint8) if isinstance(blob, (bytes, bytearray, memoryview)) else blob, dtype=np.uint8).reshape(-1)
    a = {name: np.ascontiguousarray(powers[name], dtype=np.uint64).reshape(-1, 8 * group) for name, group in _LAGRANGE_ARRAYS + (("beta_g2", 2),)}
    n_pow = min(a["tau_g2"].shape[0], a["alpha_g1"].shape[0], a["beta_g1"].shape[0])
    if a["beta_g2"].shape[0] < 1:
        raise L.VimzError(L.ERR_INVALID, "verify_key_origin: the string has no beta_g2")
    if verify_powers:
        n = int.from_bytes(b[32:40].tobytes(), "little") if b.size >= 40 else 0      # the domain the key's header names
        if n < 2 or n > n_pow or 2 * n - 1 > a["tau_g1"].shape[0]:
            raise L.VimzError(L.ERR_INVALID, f"verify_key_origin: the key's domain is {n}, the string holds {n_pow} powers ({a['tau_g1'].shape[0]} of tau in G1)")
        require_good_powers(ctx, powers, n, "verify_key_origin")
    vp = C.c_void_p
    result, first, sec = C.c_uint32(0), np.zeros(2, dtype=np.uint64), (C.c_double * 5)()
    fn = ctx.lib.vimz_decider_key_verify_origin
    fn.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, vp, vp, vp, C.c_size_t, vp, C.c_int, C.POINTER(C.c_uint32), vp, C.POINTER(C.c_double)]
    ctx._chk(fn(prover.h, _ptr(b), b.size, _ptr(a["tau_g1"]), a["tau_g1"].shape[0], _ptr(a["tau_g2"]), _ptr(a["alpha_g1"]), _ptr(a["beta_g1"]), n_pow, _ptr(a["beta_g2"]), L.FORM_MONTGOMERY,
                 C.byref(result), _ptr(first), sec))
    if seconds is not None:
        seconds[:] = list(sec)
    return int(result.value), (int(first[0]), int(first[1]))


def keyorigin_problems(bits):
    """the names of an origin verdict's bits"""
    return [name for bit, name in KEYORIGIN_BITS.items() if bits & bit]


PACK_BITS = {0x1: "a coordinate is not below q", 0x2: "INF together with another bit, or a stray top bit in a G2 word 3", 0x4: "a point is not on its curve"}      # VIMZ_PACK_*
PACK_BIT_NAMES = ("COORD", "FLAGS", "OFF_CURVE")
PACKED_KEY_MAGIC, PLAIN_KEY_MAGIC = b"VG16KPK1", b"VG16KEY2"


def pack_problems(bits):
    """the names of a packing verdict's bits"""
    return [name for bit, name in PACK_BITS.items() if bits & bit]


def _as_u8(x):
    return np.ascontiguousarray(np.frombuffer(bytes(x), dtype=np.uint8) if isinstance(x, (bytes, bytearray, memoryview)) else x, dtype=np.uint8).reshape(-1)


def _points_call(ctx, name, group, a, words_out, form, seconds, who):
    n = a.shape[0]
    out = np.zeros((n, words_out), dtype=np.uint64)
    vp = C.c_void_p
    result, first, sec = C.c_uint32(0), C.c_uint64(0), (C.c_double * 2)()
    fn = getattr(ctx.lib, name)
    fn.argtypes = [vp, C.c_int, vp, C.c_size_t, C.c_int, vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
    keep = (np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint64))      # (n = 0: the pointers must still be non-NULL)
    ctx._chk(fn(ctx.h, int(group), _ptr(a) if n else _ptr(keep[0]), n, int(form), _ptr(out) if n else _ptr(keep[1]), C.byref(result), C.byref(first), sec))
    if seconds is not None:
        seconds[:] = list(sec)
    if result.value:
        raise L.VimzError(L.ERR_INVALID, f"{who}: point {int(first.value)} is refused: " + "; ".join(pack_problems(result.value)) +
                          f" ({' | '.join(n for k, n in enumerate(PACK_BIT_NAMES) if result.value >> k & 1)} at {int(first.value)})")
    return out


def pack_points(ctx, group, points, form=L.FORM_CANONICAL, seconds=None):
    """vimz_points_pack: n affine points of G1 (group 1: rows of 8 uint64 words, x then y) or G2 (group 2: rows of 16, x.c0 x.c1 y.c0 y.c1) in `form`, the identity as
    zeros, to the packed encoding of include/vimz_hip.h — x and one bit of y, half the bytes, always canonical — on the GPU.  Returns rows of 4 (G1) or 8 (G2) words.
    seconds: a list that receives [host, device with copies].  VimzError(ERR_INVALID) naming the finding (PACK_BITS) and the first point that has one: a coordinate not
    below q, a point off its curve."""
    if group not in (1, 2):
        raise L.VimzError(L.ERR_INVALID, "pack_points: group is 1 (G1) or 2 (G2)")
    a = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 8 * group)
    return _points_call(ctx, "vimz_points_pack", group, a, 4 * group, form, seconds, "pack_points")


def unpack_points(ctx, group, packed, form=L.FORM_CANONICAL, seconds=None):
    """vimz_points_unpack: the other way — y is a square root of x³ + b taken on the GPU, so a point that unpacks is on its curve (membership of G2's subgroup is NOT
    judged: that stays with verify_powers, verify_key_origin and Decider.load_key).  packed: rows of 4 (G1) or 8 (G2) words; returns rows of 8 or 16 in `form`.
    VimzError(ERR_INVALID) naming the finding and the first point that has one: a coordinate not below q, bad flag bits, an x with no y."""
    if group not in (1, 2):
        raise L.VimzError(L.ERR_INVALID, "unpack_points: group is 1 (G1) or 2 (G2)")
    a = np.ascontiguousarray(packed, dtype=np.uint64).reshape(-1, 4 * group)
    return _points_call(ctx, "vimz_points_unpack", group, a, 8 * group, form, seconds, "unpack_points")


def key_is_packed(blob):
    """does the blob start with a packed key's magic?  (Nothing else is looked at.)"""
    return bytes(_as_u8(blob)[:8]) == PACKED_KEY_MAGIC


def _key_call(ctx, name, blob, who):
    b = _as_u8(blob)
    vp = C.c_void_p
    fn = getattr(ctx.lib, name)
    fn.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_uint32), vp]
    fn.restype = C.c_int64
    result, first = C.c_uint32(0), np.zeros(2, dtype=np.uint64)
    n = fn(ctx.h, _ptr(b), b.size, None, 0, C.byref(result), _ptr(first))
    if n < 0:
        ctx._chk(int(n))
    out = np.zeros(n, dtype=np.uint8)
    got = fn(ctx.h, _ptr(b), b.size, _ptr(out), n, C.byref(result), _ptr(first))
    if got != n:
        ctx._chk(int(got) if got < 0 else L.ERR_INVALID)
    if result.value:
        raise L.VimzError(L.ERR_INVALID, f"{who}: the point at word {int(first[0])} of the blob is refused: " + "; ".join(pack_problems(result.value)) +
                          f" ({' | '.join(n for k, n in enumerate(PACK_BIT_NAMES) if result.value >> k & 1)} at word {int(first[0])})")
    return out


def pack_key(ctx, blob):
    """vimz_decider_key_pack: a saved decider key (Decider.save_key's bytes) in half the bytes — the header verbatim under the magic "VG16KPK1", every point packed,
    the queries on the GPU.  Needs a context, no prover.  Returns a uint8 array.  VimzError(ERR_INVALID): not a key, or a point of it with a coordinate not below q or
    off its curve (the message names the point's word offset in the blob)."""
    return _key_call(ctx, "vimz_decider_key_pack", blob, "pack_key")


def unpack_key(ctx, blob):
    """vimz_decider_key_unpack: Decider.save_key's bytes from a packed key, byte for byte — every point on its curve by construction.  VimzError(ERR_INVALID): not a
    packed key, or a point that does not unpack."""
    return _key_call(ctx, "vimz_decider_key_unpack", blob, "unpack_key")


def _plain_key(ctx, blob):
    """(the key in Decider.save_key's layout, whether it came packed)"""
    return (unpack_key(ctx, blob), True) if key_is_packed(blob) else (blob, False)


def set_head_rows(rows):
    """vimz_set_head_rows: rows of a short fold call whose Poseidon chains run on the host (0: all on the GPU; -1: the library's policy)."""
    lib = L.lib()
    lib.vimz_set_head_rows.argtypes = [C.c_long]
    lib.vimz_set_head_rows.restype = C.c_long
    return int(lib.vimz_set_head_rows(int(rows)))


def set_rows_group(rows):
    """vimz_set_rows_group: the most rows of a batch whose witness commitments the producer issues as one chain of launches (0 / 1: per row; -1: the default)."""
    lib = L.lib()
    lib.vimz_set_rows_group.argtypes = [C.c_long]
    lib.vimz_set_rows_group.restype = C.c_long
    return int(lib.vimz_set_rows_group(int(rows)))


class Decider:
    """vimz_decider: `Decider::preprocess` / `prove` / `verify` of the Sonobe backend (vimz/src/sonobe_backend/mod.rs:72-80) — the 25 calldata words of
    contracts/*Verifier.sol and their local verification.  prover: a CycleFoldIVC (shapes, keys, context; keep it open); kzg_vk: [tau]G2 of the SRS
    its ck_main is made of (kzg_setup), or None (no verify).  light=False: the FULL decider (decider.rs:13-21: the running CycleFold instance's commitments
    and relation are checked inside the circuit); light=True: the reference's opt-in `light-test` variant (vimz/Cargo.toml:56-59).  The Groth16 trapdoor is drawn from the OS's randomness and forgotten; `seed` selects
    the deterministic TEST setup of libvimz_hip_testing.so.
    powers: iden3.read_ptau's dictionary instead — vimz_decider_setup_from_powers: the key is derived on the GPU from the string's points, so tau, alpha and beta
    are the string's and never in this process, gamma = 1, and only delta is drawn here (and forgotten).  kzg_vk is then the string's tau_g2[1] — passing one as
    well is refused — and the prover's ck_main must come from the same string (kzg_from_powers).  `delta` (an int; with powers only) selects the TEST set-up of
    libvimz_hip_testing.so with that delta.  verify_powers=True (with powers only): the prefix the set-up reads — the circuit's domain n of tau_g2, alpha_g1, beta_g1
    and 2n − 1 of tau_g1 — goes through hip.verify_powers first, and a refused string raises VimzError(ERR_INVALID) naming the problems before any key is made."""
    RESULT_BITS = {1: "fewer than two steps", 2: "KZG opening of cmW", 4: "KZG opening of cmE", 8: "Groth16", 16: "a word pair is not a curve point"}

    def __init__(self, prover, kzg_vk=None, seed=None, light=False, powers=None, delta=None, verify_powers=False):
        if powers is not None and (kzg_vk is not None or seed is not None):
            raise L.VimzError(L.ERR_INVALID, "Decider: powers= brings its own KZG verifying key (the string's tau_g2[1]) and draws no trapdoor: pass neither kzg_vk= nor seed= with it")
        if delta is not None and powers is None:
            raise L.VimzError(L.ERR_INVALID, "Decider: delta= goes with powers= only")
        if verify_powers and powers is None:
            raise L.VimzError(L.ERR_INVALID, "Decider: verify_powers= goes with powers= only")
        self.prover, self.ctx = prover, prover.ctx
        self.light = bool(light)
        lib = self.ctx.lib
        vp = C.c_void_p
        lib.vimz_decider_setup.argtypes = [vp, vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_double)]
        lib.vimz_decider_free.argtypes = [vp]
        lib.vimz_decider_free.restype = None
        lib.vimz_decider_info.argtypes = [vp, vp]
        lib.vimz_decider_vk.argtypes = [vp, vp, C.c_size_t]
        lib.vimz_decider_vk.restype = C.c_int64
        lib.vimz_decider_prove.argtypes = [vp, vp, vp, vp, C.POINTER(C.c_double)]
        lib.vimz_decider_verify.argtypes = [vp, C.c_uint64, vp, vp, vp, C.POINTER(C.c_uint32)]
        if powers is not None:
            if verify_powers:
                lib.vimz_decider_domain.argtypes = [vp, C.c_int, C.POINTER(C.c_uint64)]
                domain = C.c_uint64(0)
                self.ctx._chk(lib.vimz_decider_domain(prover.h, int(self.light), C.byref(domain)))
                require_good_powers(self.ctx, powers, int(domain.value), "Decider")
            self._setup_from_powers(powers, delta)
            return
        h = vp()
        sec = (C.c_double * 4)()
        self._kzg_vk = None if kzg_vk is None else np.ascontiguousarray(kzg_vk, dtype=np.uint64)
        kp = None if self._kzg_vk is None else _ptr(self._kzg_vk)
        if seed is None:
            self.ctx._chk(lib.vimz_decider_setup(prover.h, kp, int(self.light), C.byref(h), sec))
        else:
            fn = _seeded(self.ctx, "vimz_testing_decider_setup_seeded")
            fn.argtypes = [vp, vp, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(vp), C.POINTER(C.c_double)]
            self.ctx._chk(fn(prover.h, kp, int(self.light), bytes(seed), len(seed), C.byref(h), sec))
        self.h = h
        self.setup_seconds = {"circuit_synthesis": sec[0], "qap_at_trapdoor_host": sec[1], "key_points_gpu": sec[2], "total": sec[3]}

    def _setup_from_powers(self, powers, delta):
        lib, vp = self.ctx.lib, C.c_void_p
        a = {name: np.ascontiguousarray(powers[name], dtype=np.uint64).reshape(-1, 8 * group) for name, group in _LAGRANGE_ARRAYS + (("beta_g2", 2),)}
        n_pow = min(a["tau_g2"].shape[0], a["alpha_g1"].shape[0], a["beta_g1"].shape[0])
        if a["beta_g2"].shape[0] < 1:
            raise L.VimzError(L.ERR_INVALID, "Decider: the string has no beta_g2")
        head = [self.prover.h, int(self.light), _ptr(a["tau_g1"]), a["tau_g1"].shape[0], _ptr(a["tau_g2"]), _ptr(a["alpha_g1"]), _ptr(a["beta_g1"]), n_pow, _ptr(a["beta_g2"]), L.FORM_MONTGOMERY]
        types = [vp, C.c_int, vp, C.c_size_t, vp, vp, vp, C.c_size_t, vp, C.c_int]
        h = vp()
        sec = (C.c_double * 6)()
        if delta is None:
            lib.vimz_decider_setup_from_powers.argtypes = types + [C.POINTER(vp), C.POINTER(C.c_double)]
            self.ctx._chk(lib.vimz_decider_setup_from_powers(*head, C.byref(h), sec))
        else:
            fn = _seeded(self.ctx, "vimz_testing_decider_setup_from_powers_delta")
            fn.argtypes = types + [vp, C.POINTER(vp), C.POINTER(C.c_double)]
            dw = np.frombuffer(int(delta).to_bytes(32, "little"), dtype="<u8").astype(np.uint64)
            self.ctx._chk(fn(*head, _ptr(dw), C.byref(h), sec))
        self.h = h
        self._kzg_vk = None      # (the library holds the string's tau_g2[1]; key_words() has it)
        self.setup_seconds = {"circuit_synthesis": sec[0], "checks_and_upload": sec[1], "transforms_gpu": sec[2], "column_sums_gpu": sec[3], "scaling_and_key_tables": sec[4],
                              "total": sec[5]}

    def close(self):
        if self.h:
            self.ctx.lib.vimz_decider_free(self.h)
            self.h = None

    def save_key(self, packed=False):
        """vimz_decider_key_save: the key pair as bytes (uint8 array; 0.5 GB at contrast HD).  packed=True: through vimz_decider_key_pack — every point as x and one
        bit of y, about half the bytes (hip.pack_key); load_key and the key calls take either form."""
        lib = self.ctx.lib
        lib.vimz_decider_key_save.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        lib.vimz_decider_key_save.restype = C.c_int64
        n = lib.vimz_decider_key_save(self.h, None, 0)
        if n < 0:
            self.ctx._chk(int(n))
        buf = np.zeros(n, dtype=np.uint8)
        got = lib.vimz_decider_key_save(self.h, _ptr(buf), n)
        if got != n:
            self.ctx._chk(int(got) if got < 0 else L.ERR_INVALID)
        return pack_key(self.ctx, buf) if packed else buf

    @classmethod
    def load_key(cls, prover, blob):
        """vimz_decider_key_load: a decider over `prover` (a CycleFoldIVC) from a saved — or externally made — key pair; no trapdoor is involved.  A packed key
        (save_key(packed=True), hip.pack_key) is unpacked on the prover's context first.  .light is the mode the key's header names."""
        blob = _plain_key(prover.ctx, blob)[0]
        d = cls.__new__(cls)
        d.prover, d.ctx = prover, prover.ctx
        lib = d.ctx.lib
        vp = C.c_void_p
        lib.vimz_decider_key_load.argtypes = [vp, vp, C.c_size_t, C.POINTER(vp)]
        lib.vimz_decider_free.argtypes = [vp]
        lib.vimz_decider_free.restype = None
        lib.vimz_decider_info.argtypes = [vp, vp]
        lib.vimz_decider_vk.argtypes = [vp, vp, C.c_size_t]
        lib.vimz_decider_vk.restype = C.c_int64
        lib.vimz_decider_prove.argtypes = [vp, vp, vp, vp, C.POINTER(C.c_double)]
        lib.vimz_decider_verify.argtypes = [vp, C.c_uint64, vp, vp, vp, C.POINTER(C.c_uint32)]
        b = np.ascontiguousarray(blob, dtype=np.uint8)
        h = vp()
        d.ctx._chk(lib.vimz_decider_key_load(prover.h, _ptr(b), b.size, C.byref(h)))
        d.h = h
        d.light = bool(int.from_bytes(b[48:56].tobytes(), "little"))      # header word 6: 0 full, 1 light
        d._kzg_vk = None
        d.setup_seconds = {"circuit_synthesis": 0.0, "qap_at_trapdoor_host": 0.0, "key_points_gpu": 0.0, "total": 0.0}
        return d

    def info(self):
        a = np.zeros(8, dtype=np.uint64)
        self.ctx._chk(self.ctx.lib.vimz_decider_info(self.h, _ptr(a)))
        return dict(zip(["constraints", "wires", "public_inputs", "domain", "nnz_a", "nnz_b", "nnz_c", "cyclefold_rows"], (int(x) for x in a[:8])))

    def key_words(self):
        """vimz_decider_vk's words (uint64 array): what vimz_decider_verify_key takes."""
        return _export(self.ctx.lib.vimz_decider_vk, self.h).view(np.uint64)

    def verifying_key(self):
        """The constants of a contract generated for this circuit, as Python integers, in the shape tests/_novadecider.py's `verify` takes:
        {"len_z", "pp_hash", "groth16": {"alpha": G1, "beta", "gamma", "delta": G2, "ic": [G1 ...]}, "kzg": {"G_1": G1, "G_2": G2, "VK": G2}};
        G2 points ((x.c0, x.c1), (y.c0, y.c1)) = (real, imaginary)."""
        return parse_verifying_key(self.key_words())

    def prove(self, ivc=None):
        """Decider::prove for the IVC proof `ivc` (default: the prover the decider was set up over) holds.  Returns (25 words: ints, public inputs:
        ints, seconds dict).  "chains_gpu": kernel and download of check 5's chains on the device (inside the first two spans; 0 when the host makes them:
        the light decider, or VIMZ_DECIDER_CHAINS=host — read per call; the default is gpu)."""
        ivc = self.prover if ivc is None else ivc
        n_pub = self.info()["public_inputs"]
        pub = np.zeros((n_pub, 4), dtype=np.uint64)
        words = np.zeros((25, 4), dtype=np.uint64)
        sec = (C.c_double * 6)()
        self.ctx._chk(self.ctx.lib.vimz_decider_prove(self.h, ivc.h, _ptr(pub), _ptr(words), sec))
        ints = lambda a: [sum(int(a[i, q]) << (64 * q) for q in range(4)) for i in range(a.shape[0])]
        return ints(words), ints(pub), {"final_fold_and_kzg": sec[0], "witness_host": sec[1], "ntt": sec[2], "msm": sec[3], "total": sec[4], "chains_gpu": sec[5]}

    def verify(self, steps, z0, z_i, words):
        """Decider::verify: 0 = accepted, else the bit set of RESULT_BITS."""
        z0a, zia, wa = _zlimbs([int(x) for x in z0], len(z0)), _zlimbs([int(x) for x in z_i], len(z_i)), _zlimbs([int(x) for x in words], 25)
        res = C.c_uint32(0)
        self.ctx._chk(self.ctx.lib.vimz_decider_verify(self.h, int(steps), _ptr(z0a), _ptr(zia), _ptr(wa), C.byref(res)))
        return int(res.value)

    def verify_batch(self, items, chunk=0, bisect=True, leaf=0, stats=None):
        """Decider::verify for many (steps, z0, z_i, words) at once, over this decider's key words and context (verify_decider_batch): the list of result bits,
        each what `verify` gives for that proof alone.  bisect, leaf, stats: as verify_decider_batch takes them."""
        return verify_decider_batch(self.ctx, self.key_words(), items, chunk=chunk, bisect=bisect, leaf=leaf, stats=stats)


def parse_verifying_key(w):
    w = [int(x) for x in w]
    pos = [0]

    def el():
        v = sum(w[pos[0] + q] << (64 * q) for q in range(4))
        pos[0] += 4
        return v

    def g1():
        return (el(), el())

    def g2():
        return ((el(), el()), (el(), el()))

    pp = el()
    len_z = w[pos[0]]
    pos[0] += 1
    alpha, beta, gamma, delta = g1(), g2(), g2(), g2()
    n_ic = w[pos[0]]
    pos[0] += 1
    ic = [g1() for _ in range(n_ic)]
    kz = {"G_1": g1(), "G_2": g2(), "VK": g2()}
    assert pos[0] == len(w)
    return {"len_z": len_z, "pp_hash": pp, "groth16": {"alpha": alpha, "beta": beta, "gamma": gamma, "delta": delta, "ic": ic}, "kzg": kz}


def verifying_key_words(key):
    """The inverse of parse_verifying_key: a key in tests/_novadecider.py's shape as the words vimz_decider_verify_key takes."""
    out = []

    def el(v):
        out.extend((int(v) >> (64 * q)) & 0xFFFFFFFFFFFFFFFF for q in range(4))

    def g1(p):
        el(p[0]); el(p[1])

    def g2(p):
        el(p[0][0]); el(p[0][1]); el(p[1][0]); el(p[1][1])

    g = key["groth16"]
    el(key["pp_hash"]); out.append(int(key["len_z"]))
    g1(g["alpha"]); g2(g["beta"]); g2(g["gamma"]); g2(g["delta"])
    out.append(len(g["ic"]))
    for p in g["ic"]:
        g1(p)
    g1(key["kzg"]["G_1"]); g2(key["kzg"]["G_2"]); g2(key["kzg"]["VK"])
    return np.array(out, dtype=np.uint64)


def decider_verify_key(key_words, steps, z0, z_i, words):
    """vimz_decider_verify_key: host only, no context, no GPU.  Returns the result bits (0 = accepted); raises VimzError on a malformed key."""
    lib = L.lib()
    vp = C.c_void_p
    lib.vimz_decider_verify_key.argtypes = [vp, C.c_size_t, C.c_uint64, vp, vp, C.c_uint32, vp, C.POINTER(C.c_uint32)]
    kw = np.ascontiguousarray(key_words, dtype=np.uint64)
    z0a, zia, wa = _zlimbs([int(x) for x in z0], len(z0)), _zlimbs([int(x) for x in z_i], len(z_i)), _zlimbs([int(x) for x in words], 25)
    res = C.c_uint32(0)
    rc = lib.vimz_decider_verify_key(_ptr(kw), kw.size, int(steps), _ptr(z0a), _ptr(zia), len(z0), _ptr(wa), C.byref(res))
    if rc:
        raise L.VimzError(rc, "vimz_decider_verify_key: malformed key or arguments")
    return int(res.value)


MLKZG_PROBLEMS = {0x1: "malformed: word count, logn, an element not below r or a coordinate not below q", 0x2: "a point is not on its curve",
                  0x4: "a fold equation between the evaluations fails", 0x8: "the pairing equation fails"}      # VIMZ_MLKZG_*
MLKZG_PHASES = ("folds", "evaluations", "divisions", "quotient_commitments")
_MLKZG_TAIL = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_double)]      # point, comm_out, eval_out, proof, cap_words, seconds


def _mlkzg_open(ctx, fn, head, point, seconds, point_first=False):
    """the common tail of the three vimz_*mlkzg_open entries: head, then (point, logn) or (logn — the last of head —, point), then the outputs"""
    logn = len(point)
    lib = ctx.lib
    lib.vimz_mlkzg_proof_words.argtypes, lib.vimz_mlkzg_proof_words.restype = [C.c_uint32], C.c_size_t
    pt = _zlimbs([int(x) for x in point], max(logn, 1))
    comm, ev = np.zeros(8, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    proof = np.zeros(max(1, lib.vimz_mlkzg_proof_words(logn)), dtype=np.uint64)
    sec = (C.c_double * 4)()
    args = tuple(head) + (_ptr(pt), logn) if point_first else tuple(head) + (_ptr(pt),)
    ctx._chk(fn(*args, _ptr(comm), _ptr(ev), _ptr(proof), lib.vimz_mlkzg_proof_words(logn), sec))
    if seconds is not None:
        seconds.update(zip(MLKZG_PHASES, list(sec)))
    return comm, sum(int(ev[k]) << (64 * k) for k in range(4)), proof


def mlkzg_verify(vk_g2, comm, point, eval, proof):
    """vimz_mlkzg_verify: host only, no context, no GPU.  vk_g2: [tau]G2 as kzg_setup returns it; comm: 8 words; point: integers; eval: an integer; proof: words.
    Returns the verdict word (0 = accepted, else one key of MLKZG_PROBLEMS)."""
    lib = L.lib()
    vp = C.c_void_p
    lib.vimz_mlkzg_verify.argtypes = [vp, vp, C.c_uint32, vp, vp, vp, C.c_size_t, C.POINTER(C.c_uint32)]
    vk, cm, pr = _u64(vk_g2).reshape(-1), _u64(comm).reshape(-1), _u64(proof).reshape(-1)
    if vk.size != 16 or cm.size != 8 or len(point) == 0:
        raise L.VimzError(L.ERR_INVALID, "mlkzg_verify: vk_g2 has 16 words, comm 8, the point one element at least")
    pt, ev = _zlimbs([int(x) for x in point], len(point)), _zlimbs([int(eval)], 1)
    res = C.c_uint32(0)
    rc = lib.vimz_mlkzg_verify(_ptr(vk), _ptr(cm), len(point), _ptr(pt), _ptr(ev), _ptr(pr), pr.size, C.byref(res))
    if rc:
        raise L.VimzError(rc, "vimz_mlkzg_verify: bad argument")
    return int(res.value)


BATCH_NO_BISECT = 1          # VIMZ_BATCH_NO_BISECT
BATCH_STATS = ("chunks_refused", "subset_equations", "single_verifications", "accepted_by_subset")


def _batch_tail(bisect, leaf):
    """(flags, leaf, stats[4]) of the batch verifiers' _ex entries"""
    return (0 if bisect else BATCH_NO_BISECT), int(leaf), (C.c_uint64 * 4)()


def verify_decider_batch(ctx, key_words, items, chunk=0, seconds=None, multipliers=None, bisect=True, leaf=0, stats=None):
    """vimz_decider_verify_batch: many proofs under one key.  items: a sequence of (steps, z0, z_i, words) as Decider.verify takes them (calldata.decode's
    "steps", "z0", "z_i", "proof").  ctx: a Context — the per-proof part runs on the GPU — or None: the same batch on the host's threads, no GPU.  Returns the list
    of result bits, each what decider_verify_key gives for that proof alone.  seconds: a dict that receives the call's split.  multipliers (tests only, testing
    library): 3 ints a proof in place of the OS's randomness.  A refused chunk is bisected down to refused subsets of at most `leaf` proofs (0: the library's
    default), which the single verifier judges; bisect=False sends it there whole.  The words are the same either way.  stats: a dict that receives BATCH_STATS."""
    lib = L.lib() if ctx is None else ctx.lib
    vp = C.c_void_p
    kw = np.ascontiguousarray(key_words, dtype=np.uint64)
    items = list(items)
    n = len(items)
    len_z = len(items[0][1]) if n else 0
    if any(len(z0) != len_z or len(zi) != len_z or len(w) != 25 for _, z0, zi, w in items):
        raise L.VimzError(L.ERR_INVALID, "verify_decider_batch: every proof has 25 words and states of one width")
    if n == 0:
        len_z = int(kw[4]) if kw.size > 4 else 0
    steps = np.array([int(s) for s, _, _, _ in items], dtype=np.uint64)
    z0a = _zlimbs([int(x) for _, z0, _, _ in items for x in z0], n * len_z)
    zia = _zlimbs([int(x) for _, _, zi, _ in items for x in zi], n * len_z)
    wa = _zlimbs([int(x) for _, _, _, w in items for x in w], n * 25)
    res = np.zeros(max(n, 1), dtype=np.uint32)
    sec = (C.c_double * 6)()
    head = [None if ctx is None else ctx.h, _ptr(kw), kw.size, len_z, n, _ptr(steps), _ptr(z0a), _ptr(zia), _ptr(wa), int(chunk)]
    types = [vp, vp, C.c_size_t, C.c_uint32, C.c_size_t, vp, vp, vp, vp, C.c_size_t]
    flags, leaf, st = _batch_tail(bisect, leaf)
    tail = [C.c_uint32, C.c_size_t, C.POINTER(C.c_uint64)]
    if multipliers is None:
        lib.vimz_decider_verify_batch_ex.argtypes = types + [vp, C.POINTER(C.c_double)] + tail
        rc = lib.vimz_decider_verify_batch_ex(*head, _ptr(res), sec, flags, leaf, st)
    else:
        fn = L.testing_lib().vimz_testing_decider_verify_batch_scalars_ex
        fn.argtypes = types + [vp, vp, C.POINTER(C.c_double)] + tail
        ma = np.frombuffer(b"".join(int(x).to_bytes(16, "little") for x in multipliers), dtype="<u8").astype(np.uint64)
        rc = fn(*head, _ptr(ma), _ptr(res), sec, flags, leaf, st)
    if rc:
        if ctx is not None:
            ctx._chk(rc)
        lib.vimz_last_error.restype = C.c_char_p
        raise L.VimzError(rc, (lib.vimz_last_error(None) or b"vimz_decider_verify_batch").decode())
    if seconds is not None:
        seconds.update(zip(("parse_and_host", "per_proof_stage", "miller_loops", "chunk_products", "fallback", "total"), (float(x) for x in sec)))
    if stats is not None:
        stats.update(zip(BATCH_STATS, (int(x) for x in st)))
    return [int(x) for x in res[:n]]


class PendingFold:
    """vimz_ivc_pending: the segments' folds of a run of rows, begun before the state they start from is known (MergedProof.fold_segments_begin)."""

    def __init__(self, merged_cls, ivcs, step_inputs):
        self.merged_cls, self.vk, self.ctx = merged_cls, ivcs[0], ivcs[0].ctx
        lib = self.ctx.lib
        vp = C.c_void_p
        lib.vimz_ivc_fold_segments_begin.argtypes = [vp, C.c_size_t, vp, C.c_size_t, C.POINTER(vp)]
        lib.vimz_ivc_pending_digests.argtypes = [vp, vp]
        lib.vimz_ivc_pending_start.argtypes = [vp, vp]
        lib.vimz_ivc_pending_finish.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_double)]
        self.rows = np.ascontiguousarray(_u64(step_inputs).reshape(-1, self.vk.circuit.n_priv, 4))      # (kept alive: the folds read it until finish)
        arr = (vp * len(ivcs))(*[v.h for v in ivcs])
        h = vp()
        self.ctx._chk(lib.vimz_ivc_fold_segments_begin(arr, len(ivcs), _ptr(self.rows), self.rows.shape[0], C.byref(h)))
        self.h = h

    def digests(self):
        """(rows, stride, 4) uint64: the rows' digests, as IVC.row_digests returns them.  Blocks until the folds' chain passes have produced them."""
        stride = self.vk.digest_stride()
        out = np.zeros((self.rows.shape[0], stride, 4), dtype=np.uint64)
        self.ctx._chk(self.ctx.lib.vimz_ivc_pending_digests(self.h, _ptr(out)))
        return out

    def start(self, z_start):
        self.ctx._chk(self.ctx.lib.vimz_ivc_pending_start(self.h, _ptr(_zlimbs(z_start, self.vk.circuit.len_z))))

    def finish(self):
        """Joins the folds and merges: (MergedProof, {"merge_s", "total_s"})."""
        h, self.h = self.h, None
        mh = C.c_void_p()
        sec = (C.c_double * 3)()
        self.ctx._chk(self.ctx.lib.vimz_ivc_pending_finish(h, C.byref(mh), sec))
        m = self.merged_cls.__new__(self.merged_cls)
        self.merged_cls.__init__(m, _handle=mh, _vk=self.vk)
        return m, {"state_chain_s": 0.0, "merge_s": sec[1], "total_s": sec[2]}

    def cancel(self):
        if self.h:
            h, self.h = self.h, None
            self.ctx.lib.vimz_ivc_pending_finish(h, None, None)


def head_rows_policy(nsteps, segments=False):
    """vimz_head_rows_policy(_segments): rows of a lone fold call of nsteps rows (segments=True: of a proof of nsteps rows made as concurrent segments) whose
    Poseidon chains the library would evaluate on the host."""
    lib = L.lib()
    fn = lib.vimz_head_rows_policy_segments if segments else lib.vimz_head_rows_policy
    fn.argtypes = [C.c_size_t]
    fn.restype = C.c_size_t
    return int(fn(int(nsteps)))


class CycleFoldMerged:
    """vimz_cf_merged: ONE proof object out of the CycleFold proofs of contiguous row segments (vimz_cf_merge).  `first`: the prover of the
    first segment (left unchanged; supplies shapes, keys and context and must stay open)."""
    PHASES = ["cross_terms_and_commitments", "folds", "host", "total"]

    def __init__(self, first=None, _handle=None, _vk=None):
        self.vk = first if first is not None else _vk
        self.ctx = self.vk.ctx
        lib = self.ctx.lib
        vp, sz = C.c_void_p, C.c_size_t
        lib.vimz_cf_merge_merged.argtypes = [vp, vp]
        lib.vimz_cf_merged_size.argtypes = [vp]
        lib.vimz_cf_merged_size.restype = sz
        lib.vimz_cf_merged_save.argtypes = [vp, vp, sz]
        lib.vimz_cf_merged_load.argtypes = [vp, vp, sz, C.POINTER(vp)]
        lib.vimz_cf_merged_create.argtypes = [vp, C.POINTER(vp)]
        lib.vimz_cf_merged_free.argtypes = [vp]
        lib.vimz_cf_merged_free.restype = None
        lib.vimz_cf_merge.argtypes = [vp, vp]
        lib.vimz_cf_merged_verify.argtypes = [vp, C.c_uint64, vp, C.POINTER(C.c_uint32)]
        lib.vimz_cf_merged_info.argtypes = [vp, vp]
        lib.vimz_cf_merged_state.argtypes = [vp, vp, vp, C.POINTER(C.c_uint64)]
        lib.vimz_cf_merged_profile.argtypes = [vp, C.POINTER(C.c_double)]
        lib.vimz_cf_merged_records.argtypes = [vp, vp, sz]
        lib.vimz_cf_merged_records.restype = C.c_int64
        lib.vimz_cf_merged_export.argtypes = [vp, C.c_int, C.c_int, vp, sz]
        lib.vimz_cf_merged_export.restype = C.c_int64
        if _handle is not None:
            self.h = _handle
            return
        h = vp()
        self.ctx._chk(lib.vimz_cf_merged_create(first.h, C.byref(h)))
        self.h = h

    @classmethod
    def load(cls, vk, blob):
        """vimz_cf_merged_load: a merged proof from bytes, into the context of `vk` (a CycleFoldIVC for the same step circuit and keys)."""
        lib = vk.ctx.lib
        lib.vimz_cf_merged_load.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
        b = np.ascontiguousarray(blob, dtype=np.uint8)
        if b.ctypes.data % 8:
            b = np.frombuffer(bytearray(b.tobytes()) + bytearray(8), dtype=np.uint8)[:b.size].copy()
        h = C.c_void_p()
        vk.ctx._chk(lib.vimz_cf_merged_load(vk.h, _ptr(b), b.size, C.byref(h)))
        return cls(_handle=h, _vk=vk)

    def save(self):
        """vimz_cf_merged_save: the object as bytes (records + folded vectors)."""
        n = self.ctx.lib.vimz_cf_merged_size(self.h)
        buf = np.zeros(n, dtype=np.uint8)
        self.ctx._chk(self.ctx.lib.vimz_cf_merged_save(self.h, _ptr(buf), n))
        return buf

    @classmethod
    def of(cls, provers):
        """The merged proof of segments proven by `provers`, in row order."""
        m = cls(provers[0])
        try:
            for v in provers[1:]:
                m.merge(v)
        except Exception:
            m.close()
            raise
        return m

    def close(self):
        if self.h:
            self.ctx.lib.vimz_cf_merged_free(self.h)
            self.h = None

    def merge(self, nxt):
        """Fold the next row segment's proof in (a CycleFoldIVC), or another merged object holding one run (vimz_cf_merge_merged)."""
        if isinstance(nxt, CycleFoldMerged):
            self.ctx._chk(self.ctx.lib.vimz_cf_merge_merged(self.h, nxt.h))
        else:
            self.ctx._chk(self.ctx.lib.vimz_cf_merge(self.h, nxt.h))

    def verify(self, num_steps, z0):
        r = C.c_uint32()
        self.ctx._chk(self.ctx.lib.vimz_cf_merged_verify(self.h, int(num_steps), _ptr(_zlimbs(z0, self.vk.circuit.len_z)), C.byref(r)))
        return r.value

    def info(self):
        a = np.zeros(8, dtype=np.uint64)
        self.ctx._chk(self.ctx.lib.vimz_cf_merged_info(self.h, _ptr(a)))
        return dict(zip(["steps", "segments", "len_z", "main_wires", "main_constraints", "cyclefold_wires", "cyclefold_constraints", "broken"], (int(x) for x in a)))

    def state(self):
        """(z_start, z_end, steps)"""
        lz = self.vk.circuit.len_z
        zs, ze = np.zeros((lz, 4), dtype=np.uint64), np.zeros((lz, 4), dtype=np.uint64)
        steps = C.c_uint64()
        self.ctx._chk(self.ctx.lib.vimz_cf_merged_state(self.h, _ptr(zs), _ptr(ze), C.byref(steps)))
        ints = lambda a: [sum(int(a[i, k]) << (64 * k) for k in range(4)) for i in range(lz)]
        return ints(zs), ints(ze), steps.value

    def profile(self):
        s = (C.c_double * 4)()
        self.ctx._chk(self.ctx.lib.vimz_cf_merged_profile(self.h, s))
        return dict(zip(self.PHASES, s))

    def share(self):
        """vimz_cf_merged_share: the ticket (records + HIP IPC handle) another process of this node opens with CycleFoldMerged.open_shared."""
        lib = self.ctx.lib
        lib.vimz_cf_merged_share.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        lib.vimz_cf_merged_share.restype = C.c_int64
        return _export(lib.vimz_cf_merged_share, self.h)

    @classmethod
    def open_shared(cls, vk, ticket):
        """vimz_cf_merged_open_shared: an object of this process's own out of another process's shared one (device-to-device copy)."""
        b = np.ascontiguousarray(np.frombuffer(bytes(ticket), dtype=np.uint8) if isinstance(ticket, (bytes, bytearray)) else ticket, dtype=np.uint8)
        lib = vk.ctx.lib
        lib.vimz_cf_merged_open_shared.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
        h = C.c_void_p()
        vk.ctx._chk(lib.vimz_cf_merged_open_shared(vk.h, _ptr(b), b.size, C.byref(h)))
        return cls(_handle=h, _vk=vk)

    def kzg_open(self, which, z):
        """vimz_cf_merged_kzg_open: (eval, proof point) of the folded main instance's comm_W (which = 0) or comm_E (1) at z."""
        lib = self.ctx.lib
        lib.vimz_cf_merged_kzg_open.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        ev, pr = np.zeros(4, dtype=np.uint64), np.zeros(8, dtype=np.uint64)
        self.ctx._chk(lib.vimz_cf_merged_kzg_open(self.h, which, _ptr(_zlimbs([z], 1)), _ptr(ev), _ptr(pr)))
        ints = lambda a: sum(int(a[k]) << (64 * k) for k in range(4))
        return ints(ev), (ints(pr[:4]), ints(pr[4:]))

    def mlkzg_open(self, which, point, seconds=None):
        """vimz_cf_merged_mlkzg_open: CycleFoldIVC.mlkzg_open for the folded main instance."""
        lib = self.ctx.lib
        lib.vimz_cf_merged_mlkzg_open.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32] + _MLKZG_TAIL[1:]
        return _mlkzg_open(self.ctx, lib.vimz_cf_merged_mlkzg_open, (self.h, which), point, seconds, point_first=True)

    def compress(self):
        """vimz_cf_merged_compress: the records and one argument each for the folded main and CycleFold instance.
        Returns (proof bytes as uint8 array, {"setup_s", "prove_s"})."""
        lib = self.ctx.lib
        lib.vimz_cf_merged_compressed_size.argtypes = [C.c_void_p]
        lib.vimz_cf_merged_compressed_size.restype = C.c_size_t
        lib.vimz_cf_merged_compress.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_double)]
        n = lib.vimz_cf_merged_compressed_size(self.h)
        buf = np.zeros(n, dtype=np.uint8)
        sec = (C.c_double * 2)()
        self.ctx._chk(lib.vimz_cf_merged_compress(self.h, _ptr(buf), n, sec))
        return buf, {"setup_s": sec[0], "prove_s": sec[1]}

    @staticmethod
    def verify_compressed(vk, blob, num_steps, z0):
        """vimz_cf_verify_merged_compressed: 0 = accepted.  vk: a CycleFoldIVC for the same step circuit and keys (the verifier key only)."""
        lib = vk.ctx.lib
        lib.vimz_cf_verify_merged_compressed.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint32)]
        b = np.ascontiguousarray(blob, dtype=np.uint8)
        r = C.c_uint32()
        vk.ctx._chk(lib.vimz_cf_verify_merged_compressed(vk.h, _ptr(b), b.size, int(num_steps), _ptr(_zlimbs(z0, vk.circuit.len_z)), C.byref(r)))
        return r.value

    def records(self):
        n = self.ctx.lib.vimz_cf_merged_records(self.h, None, 0)
        buf = np.zeros(n // 8, dtype=np.uint64)
        assert self.ctx.lib.vimz_cf_merged_records(self.h, _ptr(buf), n) == n
        return buf

    def export(self, side, what):
        return _export(self.ctx.lib.vimz_cf_merged_export, self.h, side, what).view(np.uint64).reshape(-1, 4)


def cyclefold_selfcheck(steps=4):
    """vimz_cf_selfcheck (host only, no GPU): (result bits, {"main_wires", "main_constraints", "cyclefold_wires", "cyclefold_constraints"})."""
    from . import _lib
    lib = _lib.testing_lib()
    lib.vimz_cf_selfcheck.argtypes = [C.c_int, C.POINTER(C.c_uint32), C.c_void_p]
    r = C.c_uint32()
    counts = np.zeros(8, dtype=np.uint64)
    rc = lib.vimz_cf_selfcheck(int(steps), C.byref(r), _ptr(counts))
    if rc:
        raise _lib.VimzError(rc, "vimz_cf_selfcheck")
    return r.value, dict(zip(["main_wires", "main_constraints", "cyclefold_wires", "cyclefold_constraints", "main_flipped", "main_unnoticed", "cyclefold_flipped", "cyclefold_unnoticed"],
                             (int(x) for x in counts)))


def _zlimbs(z0, len_z):
    z = np.zeros((len_z, 4), dtype=np.uint64)
    for i, v in enumerate(z0):
        for k in range(4):
            z[i, k] = (int(v) >> (64 * k)) & 0xFFFFFFFFFFFFFFFF
    return z


def _compressed_batch(vk, entry, blobs, num_steps, initial_states, chunk, multipliers=None, bisect=True, leaf=0, stats=None):
    """The shared body of IVC.verify_compressed_batch and CycleFoldIVC.verify_compressed_batch: (flag words, seconds split).  entry: the entry without _ex (its twin
    vimz_*_verify_batch_compressed*_ex is what runs).  bisect, leaf, stats: as verify_decider_batch takes them; "subset_equations" counts one a curve asked."""
    lib = vk.ctx.lib
    n = len(blobs)
    if len(num_steps) != n or len(initial_states) != n:
        raise L.VimzError(L.ERR_INVALID, f"{entry}: {n} blobs, {len(num_steps)} step counts, {len(initial_states)} initial states")
    lz = vk.circuit.len_z
    arrs = [np.ascontiguousarray(np.frombuffer(bytes(b), dtype=np.uint8) if isinstance(b, (bytes, bytearray, memoryview)) else b, dtype=np.uint8).reshape(-1) for b in blobs]
    keep = [a if a.size else np.zeros(1, dtype=np.uint8) for a in arrs]          # (an empty blob still needs an address)
    ptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in keep])
    lens = (C.c_size_t * max(n, 1))(*[a.size for a in arrs])
    steps = np.array([int(x) for x in num_steps], dtype=np.uint64)
    z = np.zeros((max(n, 1), lz, 4), dtype=np.uint64)
    for i, z0 in enumerate(initial_states):
        z[i] = _zlimbs(z0, lz)
    res = np.zeros(max(n, 1), dtype=np.uint32)
    sec = (C.c_double * 6)()
    vp, sz = C.c_void_p, C.c_size_t
    fn = getattr(lib, entry.replace("verify_compressed_batch", "verify_batch_compressed") + "_ex")
    flags, leaf, st = _batch_tail(bisect, leaf)
    tail = [C.c_uint32, sz, C.POINTER(C.c_uint64)]
    if multipliers is None:
        fn.argtypes = [vp, sz, vp, vp, vp, vp, sz, vp, C.POINTER(C.c_double)] + tail
        rc = fn(vk.h, n, ptrs, lens, _ptr(steps), _ptr(z), int(chunk), _ptr(res), sec, flags, leaf, st)
    else:
        m = np.ascontiguousarray(multipliers, dtype=np.uint64).reshape(-1)
        fn.argtypes = [vp, sz, vp, vp, vp, vp, sz, vp, vp, C.POINTER(C.c_double)] + tail
        rc = fn(vk.h, n, ptrs, lens, _ptr(steps), _ptr(z), int(chunk), _ptr(m), _ptr(res), sec, flags, leaf, st)
    vk.ctx._chk(rc)
    if stats is not None:
        stats.update(zip(BATCH_STATS, (int(x) for x in st)))
    names = ("parse_and_host_checks_s", "tables_s", "matrix_evaluation_s", "svec_accumulation_s", "msm_s", "fallback_s")
    return [int(x) for x in res[:n]], dict(zip(names, list(sec)))


class MergedProof:
    """vimz_ivc_merged: ONE proof object out of the IVC proofs of contiguous row segments (the host-side sequential final fold of
    BASELINE.json's north_star; the reference's fold_input returns one RecursiveSNARK, vimz/src/nova_snark_backend/folding.rs:27-43).
    `first`: the IVC of the first segment (left unchanged; supplies shapes, keys and context and must stay open)."""
    PHASES = ["leaf", "wait_cross_term_msm", "folds_and_host", "total"]

    def __init__(self, first=None, _handle=None, _vk=None):
        self.vk = first if first is not None else _vk
        self.ctx = self.vk.ctx
        lib = self.ctx.lib
        vp, sz = C.c_void_p, C.c_size_t
        lib.vimz_ivc_merged_create.argtypes = [vp, C.POINTER(vp)]
        lib.vimz_ivc_merged_free.argtypes = [vp]
        lib.vimz_ivc_merged_free.restype = None
        lib.vimz_ivc_merge.argtypes = [vp, vp]
        lib.vimz_ivc_merge_merged.argtypes = [vp, vp]
        lib.vimz_ivc_merged_verify.argtypes = [vp, C.c_uint64, vp, C.POINTER(C.c_uint32)]
        lib.vimz_ivc_merged_info.argtypes = [vp, vp]
        lib.vimz_ivc_merged_state.argtypes = [vp, vp, vp, C.POINTER(C.c_uint64)]
        lib.vimz_ivc_merged_profile.argtypes = [vp, C.POINTER(C.c_double)]
        lib.vimz_ivc_merged_size.argtypes = [vp]
        lib.vimz_ivc_merged_size.restype = sz
        lib.vimz_ivc_merged_save.argtypes = [vp, vp, sz]
        lib.vimz_ivc_merged_load.argtypes = [vp, vp, sz, C.POINTER(vp)]
        lib.vimz_ivc_merged_records.argtypes = [vp, vp, sz]
        lib.vimz_ivc_merged_records.restype = C.c_int64
        lib.vimz_ivc_merged_export.argtypes = [vp, C.c_int, C.c_int, vp, sz]
        lib.vimz_ivc_merged_export.restype = C.c_int64
        lib.vimz_ivc_merged_compressed_size.argtypes = [vp]
        lib.vimz_ivc_merged_compressed_size.restype = sz
        lib.vimz_ivc_merged_compress.argtypes = [vp, vp, sz, C.POINTER(C.c_double)]
        lib.vimz_ivc_verify_merged_compressed.argtypes = [vp, vp, sz, C.c_uint64, vp, C.POINTER(C.c_uint32)]
        if _handle is not None:
            self.h = _handle
        else:
            h = vp()
            self.ctx._chk(lib.vimz_ivc_merged_create(first.h, C.byref(h)))
            self.h = h

    @classmethod
    def of(cls, ivcs):
        """The merged proof of the segments' IVCs, in row order."""
        m = cls(ivcs[0])
        try:
            for v in ivcs[1:]:
                m.merge(v)
        except Exception:
            m.close()
            raise
        return m

    @classmethod
    def fold_segments(cls, ivcs, step_inputs, z0, digests=None):
        """vimz_ivc_fold_segments: fold_input in one call — the rows as len(ivcs) concurrent segments (own context each), merged.
        digests (optional): the rows' digests as vimz_ivc_row_digests returns them, when the caller has them already.
        Returns (MergedProof, {"state_chain_s", "merge_s", "total_s"}); its verifier key is ivcs[0]."""
        vk = ivcs[0]
        lib = vk.ctx.lib
        lib.vimz_ivc_fold_segments_dg.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_double)]
        a = _u64(step_inputs).reshape(-1, vk.circuit.n_priv, 4)
        arr = (C.c_void_p * len(ivcs))(*[v.h for v in ivcs])
        h = C.c_void_p()
        sec = (C.c_double * 3)()
        dg = None
        if digests is not None:
            dg = np.ascontiguousarray(digests, dtype=np.uint64)
            if dg.size != a.shape[0] * vk.digest_stride() * 4:
                raise ValueError("fold_segments: digests do not match the rows")
        vk.ctx._chk(lib.vimz_ivc_fold_segments_dg(arr, len(ivcs), _ptr(_zlimbs(z0, vk.circuit.len_z)), _ptr(a), a.shape[0], _ptr(dg) if dg is not None else None, C.byref(h), sec))
        m = cls.__new__(cls)
        cls.__init__(m, _handle=h, _vk=vk)
        return m, {"state_chain_s": sec[0], "merge_s": sec[1], "total_s": sec[2]}

    @classmethod
    def fold_segments_begin(cls, ivcs, step_inputs):
        """vimz_ivc_fold_segments_begin: fold_input for a run of rows whose start state is not known yet (a rank of a sharded proof).  Returns a
        PendingFold: .digests() blocks until the rows are hashed (by the folds' own chain passes), .start(z) provides the state, .finish() -> (MergedProof, seconds)."""
        return PendingFold(cls, ivcs, step_inputs)

    @classmethod
    def load(cls, vk, blob):
        """vimz_ivc_merged_load: `vk` = an IVC for the same step circuit and keys (its state is not touched)."""
        b = np.ascontiguousarray(blob, dtype=np.uint8)
        m = cls.__new__(cls)
        cls.__init__(m, _handle=C.c_void_p(0), _vk=vk)
        h = C.c_void_p()
        vk.ctx._chk(vk.ctx.lib.vimz_ivc_merged_load(vk.h, _ptr(b), b.size, C.byref(h)))
        m.h = h
        return m

    def share(self):
        """vimz_ivc_merged_share: the ticket (records + HIP IPC handle of the device allocation) another process of this node opens
        with MergedProof.open_shared; keep this object open until that process is done."""
        lib = self.ctx.lib
        lib.vimz_ivc_merged_share.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        lib.vimz_ivc_merged_share.restype = C.c_int64
        return _export(lib.vimz_ivc_merged_share, self.h)

    @classmethod
    def open_shared(cls, vk, ticket):
        """vimz_ivc_merged_open_shared: an object of this process's own out of another process's shared one (device-to-device copy)."""
        b = np.ascontiguousarray(np.frombuffer(bytes(ticket), dtype=np.uint8) if isinstance(ticket, (bytes, bytearray)) else ticket, dtype=np.uint8)
        m = cls.__new__(cls)
        cls.__init__(m, _handle=C.c_void_p(0), _vk=vk)
        lib = vk.ctx.lib
        lib.vimz_ivc_merged_open_shared.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
        h = C.c_void_p()
        vk.ctx._chk(lib.vimz_ivc_merged_open_shared(vk.h, _ptr(b), b.size, C.byref(h)))
        m.h = h
        return m

    def close(self):
        if self.h:
            self.ctx.lib.vimz_ivc_merged_free(self.h)
            self.h = None

    def merge(self, nxt):
        """Fold the next row segment in: an IVC (vimz_ivc_merge) or another merged proof (vimz_ivc_merge_merged)."""
        if isinstance(nxt, MergedProof):
            self.ctx._chk(self.ctx.lib.vimz_ivc_merge_merged(self.h, nxt.h))
        else:
            self.ctx._chk(self.ctx.lib.vimz_ivc_merge(self.h, nxt.h))

    def verify(self, num_steps, z0):
        r = C.c_uint32()
        self.ctx._chk(self.ctx.lib.vimz_ivc_merged_verify(self.h, int(num_steps), _ptr(_zlimbs(z0, self.vk.circuit.len_z)), C.byref(r)))
        return r.value

    def info(self):
        a = np.zeros(8, dtype=np.uint64)
        self.ctx._chk(self.ctx.lib.vimz_ivc_merged_info(self.h, _ptr(a)))
        keys = ["steps", "segments", "ops", "len_z", "primary_wires", "primary_constraints", "secondary_wires", "secondary_constraints"]
        return {k: int(a[i]) for i, k in enumerate(keys)}

    def state(self):
        """(z_start, z_end, steps)"""
        lz = self.vk.circuit.len_z
        a, b = np.zeros((lz, 4), dtype=np.uint64), np.zeros((lz, 4), dtype=np.uint64)
        n = C.c_uint64()
        self.ctx._chk(self.ctx.lib.vimz_ivc_merged_state(self.h, _ptr(a), _ptr(b), C.byref(n)))
        ints = lambda z: [sum(int(z[i, k]) << (64 * k) for k in range(4)) for i in range(lz)]
        return ints(a), ints(b), n.value

    def profile(self):
        s = (C.c_double * 4)()
        self.ctx._chk(self.ctx.lib.vimz_ivc_merged_profile(self.h, s))
        return {k: s[i] for i, k in enumerate(self.PHASES)}

    def save(self):
        n = self.ctx.lib.vimz_ivc_merged_size(self.h)
        buf = np.zeros(n, dtype=np.uint8)
        self.ctx._chk(self.ctx.lib.vimz_ivc_merged_save(self.h, _ptr(buf), n))
        return buf

    def records(self):
        """The statement part as uint64 words (header, segment records, ops): what an independent verifier replays."""
        return _export(self.ctx.lib.vimz_ivc_merged_records, self.h).view(np.uint64)

    def export(self, side, what):
        return _export(self.ctx.lib.vimz_ivc_merged_export, self.h, side, what).view(np.uint64).reshape(-1, 4)

    def compress(self):
        lib = self.ctx.lib
        n = lib.vimz_ivc_merged_compressed_size(self.h)
        buf = np.zeros(n, dtype=np.uint8)
        sec = (C.c_double * 2)()
        self.ctx._chk(lib.vimz_ivc_merged_compress(self.h, _ptr(buf), n, sec))
        return buf, {"setup_s": sec[0], "prove_s": sec[1]}

    @staticmethod
    def verify_compressed(vk, blob, num_steps, z0):
        lib = vk.ctx.lib
        lib.vimz_ivc_verify_merged_compressed.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint32)]
        b = np.ascontiguousarray(blob, dtype=np.uint8)
        r = C.c_uint32()
        vk.ctx._chk(lib.vimz_ivc_verify_merged_compressed(vk.h, _ptr(b), b.size, int(num_steps), _ptr(_zlimbs(z0, vk.circuit.len_z)), C.byref(r)))
        return r.value


class AugCircuit:
    """vimz_augcircuit: one side's verifier circuit over a trivial step circuit — host-only hook for the circuit's own tests."""

    def __init__(self, side):
        lib = L.lib()
        vp = C.c_void_p
        lib.vimz_augcircuit_build.argtypes = [C.c_int, C.POINTER(vp)]
        lib.vimz_augcircuit_free.argtypes = [vp]
        lib.vimz_augcircuit_free.restype = None
        lib.vimz_augcircuit_export.argtypes = [vp, C.c_int, vp, C.c_size_t]
        lib.vimz_augcircuit_export.restype = C.c_int64
        lib.vimz_augcircuit_witness.argtypes = [vp, vp, vp, vp]
        self.lib, self.side = lib, side
        h = vp()
        rc = lib.vimz_augcircuit_build(side, C.byref(h))
        if rc:
            raise L.VimzError(rc, "vimz_augcircuit_build")
        self.h = h
        info = _export(lib.vimz_augcircuit_export, self.h, IX_INFO).view(np.uint64)
        self.n_wires, self.n_constraints = int(info[0]), int(info[1])

    def close(self):
        if self.h:
            self.lib.vimz_augcircuit_free(self.h)
            self.h = None

    def r1cs(self):
        return _r1cs_tables(self.lib.vimz_augcircuit_export, self.h)

    def witness(self, inputs):
        """inputs: 17 integers (digest, i, z0, z, U[7], u[4], T[2]).  Returns (wires[n_wires] ints as (n,4) u64, outputs: list of 11 ints)."""
        a = np.zeros((17, 4), dtype=np.uint64)
        assert len(inputs) == 17
        for i, v in enumerate(inputs):
            for k in range(4):
                a[i, k] = (int(v) >> (64 * k)) & 0xFFFFFFFFFFFFFFFF
        wires = np.zeros((self.n_wires, 4), dtype=np.uint64)
        out = np.zeros((11, 4), dtype=np.uint64)
        rc = self.lib.vimz_augcircuit_witness(self.h, _ptr(a), _ptr(wires), _ptr(out))
        if rc:
            raise L.VimzError(rc, "vimz_augcircuit_witness")
        return wires, [sum(int(out[i, k]) << (64 * k) for k in range(4)) for i in range(11)]


class _Coo(C.Structure):
    _fields_ = [("row", C.c_void_p), ("col", C.c_void_p), ("val", C.c_void_p), ("nnz", C.c_size_t)]


def vec_axpy(ctx, x1, r, x2, n=None, form=L.FORM_CANONICAL):
    """x1 <- x1 + r * x2 (vimz_vec_axpy): RelaxedR1CSWitness::fold of a resident vector; r an int (canonical) or 4 limbs in `form`."""
    lib = ctx.lib
    lib.vimz_vec_axpy.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    rl = _u64([(int(r) >> (64 * i)) & ((1 << 64) - 1) for i in range(4)]) if isinstance(r, int) else _u64(r)
    ctx._chk(lib.vimz_vec_axpy(ctx.h, x1.h, rl.ctypes.data, form, x2.h, x1.n if n is None else n))


class R1CSShape:
    """vimz_r1cs: a caller-supplied R1CS shape resident on the GPU — the `R1CSShape` of nova-snark 0.23.0 behind the C ABI
    (multiply_vec -> spmv3, commit_T -> commit_T).  Matrices are COO triplets (row, col, value) in any order, like the crate's."""

    def __init__(self, ctx, field, nrows, ncols, A, B, Cm, form=L.FORM_CANONICAL):
        """A, B, Cm: (rows uint32[nnz], cols uint32[nnz], vals (nnz, 4) uint64)."""
        self.ctx, self.field, self.nrows, self.ncols = ctx, field, nrows, ncols
        lib = ctx.lib
        vp = C.c_void_p
        lib.vimz_r1cs_upload.argtypes = [vp, C.c_int, C.c_size_t, C.c_size_t, C.POINTER(_Coo), C.POINTER(_Coo), C.POINTER(_Coo), C.c_int, C.POINTER(vp)]
        lib.vimz_r1cs_free.argtypes = [vp, vp]
        lib.vimz_r1cs_free.restype = None
        lib.vimz_spmv3.argtypes = [vp, vp, vp, vp, vp, vp]
        lib.vimz_r1cs_info.argtypes = [vp, vp]
        lib.vimz_commit_T.argtypes = [vp, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, C.c_int]
        keep, coos = [], []
        for rows, cols, vals in (A, B, Cm):
            r, c = np.ascontiguousarray(rows, dtype=np.uint32), np.ascontiguousarray(cols, dtype=np.uint32)
            v = _u64(vals)
            keep += [r, c, v]
            coos.append(_Coo(r.ctypes.data, c.ctypes.data, v.ctypes.data, r.size))
        h = vp()
        ctx._chk(lib.vimz_r1cs_upload(ctx.h, field, nrows, ncols, C.byref(coos[0]), C.byref(coos[1]), C.byref(coos[2]), form, C.byref(h)))
        self.h = h

    def check_relaxed(self, z, u, E=None, form=L.FORM_CANONICAL):
        """is_sat_relaxed (vimz_r1cs_check_relaxed): (number of unsatisfied rows, first of them or None)."""
        lib = self.ctx.lib
        lib.vimz_r1cs_check_relaxed.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        ul = _u64([(int(u) >> (64 * i)) & ((1 << 64) - 1) for i in range(4)]) if isinstance(u, int) else _u64(u)
        bad, first = C.c_uint64(), C.c_uint64()
        self.ctx._chk(lib.vimz_r1cs_check_relaxed(self.ctx.h, self.h, z.h, ul.ctypes.data, form, E.h if E is not None else None, C.byref(bad), C.byref(first)))
        return int(bad.value), (int(first.value) if bad.value else None)

    def free(self):
        if self.h:
            self.ctx.lib.vimz_r1cs_free(self.ctx.h, self.h)
            self.h = None

    def multiply_vec(self, z, out=None):
        """R1CSShape::multiply_vec: z a DeviceVec of ncols elements -> (Az, Bz, Cz), as new DeviceVecs or in the caller's three `out`
        (each of at least nrows elements; what lies beyond nrows is left alone)."""
        out = [self.ctx.vec_alloc(self.field, self.nrows) for _ in range(3)] if out is None else list(out)
        self.ctx._chk(self.ctx.lib.vimz_spmv3(self.ctx.h, self.h, z.h, out[0].h, out[1].h, out[2].h))
        return out

    def commit_T(self, ck, z1, u1, z2, u2=1, out=None, form=L.FORM_CANONICAL):
        """R1CSShape::commit_T: returns (T DeviceVec of nrows elements — a new one, or the caller's `out` — and comm_T as (8,) uint64
        canonical affine); u1, u2 integers in `form`."""
        T = self.ctx.vec_alloc(self.field, self.nrows) if out is None else out
        lim = lambda x: np.array([(int(x) >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)], dtype=np.uint64)
        a, b = lim(u1), lim(u2)
        res = np.zeros(8, dtype=np.uint64)
        try:
            self.ctx._chk(self.ctx.lib.vimz_commit_T(self.ctx.h, self.h, ck.h, z1.h, _ptr(a), z2.h, _ptr(b), form, T.h, _ptr(res), L.FORM_CANONICAL))
        except Exception:
            if out is None:
                T.free()
            raise
        return T, res

    def info(self):
        """vimz_r1cs_info: rows, columns, non-zeros of A, B, C, dictionary size, long (matrix, row) items, field."""
        a = np.zeros(8, dtype=np.uint64)
        self.ctx._chk(self.ctx.lib.vimz_r1cs_info(self.h, _ptr(a)))
        return dict(zip(("nrows", "ncols", "nnz_a", "nnz_b", "nnz_c", "dict", "n_long", "field"), (int(x) for x in a)))
