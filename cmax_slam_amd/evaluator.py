"""Host-side mirror of the reference's evaluator interface over the C ABI (include/cmax_hip.h).

Names follow the reference so the parity tests read like its own call sites:

  FrontendEvaluator  <->  cmax_slam::AngVelEstimator's hot-path members
      set_packet                     event_subset_ / time_packet_ hand-over   (ang_vel_estimator.cpp:137-147)
      computeImageOfWarpedEvents     local_image_warped_events.cpp:10-57
      contrast_f / contrast_df / contrast_fdf   local_contrast_{f,df,fdf}   (local_optim_contrast_gsl.cpp:20-70)

  BackendEvaluator   <->  PoseGraphOptimizer + EventWarper hot-path members
      set_window                     processTimeWindow hand-over             (pose_graph_optimizer.cpp:283-293)
      computeImageOfWarpedEvents     event_pano_warper.cpp:167-231
      contrast_f / contrast_df / contrast_fdf   global_contrast_{f,df,fdf}  (global_optim_contrast_gsl_analytical.cpp:17-81)

contrast_* return the GSL-side values: f = -contrast, df = -gradient.  eval() returns the un-negated pair.
All compute happens in libcmaxhip.so's HIP kernels; numpy only carries host buffers across the ABI.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import (GRAD_ADJOINT, GRAD_PLANES, MEAN_SQUARE, VARIANCE, CmaxHipError, c_dp, c_fp, c_i64p, c_u16p,
                   check)

__all__ = ["FrontendEvaluator", "BackendEvaluator", "EventStore", "CmaxHipError", "VARIANCE", "MEAN_SQUARE", "GRAD_PLANES",
           "GRAD_ADJOINT"]


def _c(a, dt):
    return np.ascontiguousarray(a, dtype=dt)


def _dp(a):
    return a.ctypes.data_as(c_dp)


def _pol_bytes(polarity):
    """one byte per event, nonzero = ON (bool, integer or +-1 float arrays alike: > 0 is ON for signed input)"""
    p = np.asarray(polarity)
    if p.dtype == np.uint8 or p.dtype == np.bool_:
        return np.ascontiguousarray(p).view(np.uint8)
    return np.ascontiguousarray(p > 0).view(np.uint8)


def _on_device(a, name):
    """a tensor handed to a *_device call of the event store lives in device memory (an object that cannot say is taken at its word)"""
    if getattr(a, "is_cuda", True) is False:
        raise ValueError("%s: a tensor in device memory expected, got one on %s" % (name, getattr(a, "device", "the host")))


def _pol_offset(ev, field):
    dt, off = ev.dtype.fields[field][:2]
    if dt.itemsize != 1:
        raise ValueError("the polarity field must be one byte wide")
    return int(off)


class _Evaluator:
    def __init__(self):
        self._L = _lib.lib()
        self._ctx = _lib.ctx_p()

    def close(self):
        if getattr(self, "_ctx", None):
            self._L.cmx_destroy(self._ctx)
            self._ctx = _lib.ctx_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, status):
        check(self._ctx, status)

    def _io_buffers(self, n):
        """Persistent ctypes in/out buffers for the eval calls (+ numpy views on them): `ndarray.ctypes.data_as` and
        fresh arrays cost ~5 us per call -- a tenth of a front-end evaluation -- and a C++ host pays none of it."""
        n = max(int(n), 1)
        if getattr(self, "_io_n", 0) != n:
            self._xb, self._gb, self._cb = (C.c_double * n)(), (C.c_double * n)(), C.c_double()
            self._xin = np.frombuffer(self._xb, dtype=np.float64)
            self._gout = np.frombuffer(self._gb, dtype=np.float64)
            self._xp, self._gp = C.cast(self._xb, c_dp), C.cast(self._gb, c_dp)
            self._cref = C.pointer(self._cb)
            self._io_n = n

    def set_option(self, key, value):
        self._ck(self._L.cmx_set_option(self._ctx, int(key), int(value)))

    def set_grad_mode(self, mode):
        self.set_option(_lib.OPT_GRAD_MODE, mode)

    def set_splat_mode(self, mode):
        """0 = global atomics, 1 = LDS-privatised (events sorted by destination tile)."""
        self.set_option(_lib.OPT_SPLAT_MODE, mode)

    def stats(self):
        s = np.zeros(23)
        self._ck(self._L.cmx_get_stats(self._ctx, _dp(s), 23))
        return {"rebins": int(s[0]), "fallback_frac": float(s[1]), "chunks": int(s[2]), "events": int(s[3]),
                "reuse_hits": int(s[4]), "sharded_host_syncs": int(s[5]), "exchange_misses": int(s[6]), "exchange_tiles": int(s[7]), "comm_bytes": int(s[8]), "spec_images": int(s[9]), "spec_hits": int(s[10]),
                "gated_launches": int(s[11]), "gated_hits": int(s[12]), "chain_solves": int(s[13]), "chain_slots": int(s[14]),
                "chain_takeovers": int(s[15]), "chain_warm_starts": int(s[16]), "fused_evals": int(s[17]), "fused_redos": int(s[18]), "one_launch_evals": int(s[19]), "fused_timeouts": int(s[20]), "self_serve_evals": int(s[21]),
                "host_finalize_evals": int(s[22])}

    def _adjoint_plane(self, which, H, W):
        out = np.empty((H, W), np.float32)
        self._ck(self._L.cmx_diag_get_adjoint_plane(self._ctx, int(which), out.ctypes.data_as(c_fp)))
        return out

    def hint_next_df(self, threshold, mode):
        """cmx_hint_next_df: the next cost-only evaluation's value f = -contrast decides (mode 1: f < threshold, 2: f <= threshold,
        3: not f >= threshold, 4: always) whether the gradient pass is queued behind it."""
        self._ck(self._L.cmx_hint_next_df(self._ctx, float(threshold), int(mode)))

    def set_fast_path(self):
        """The production configuration and the library's default: adjoint gradient + LDS-privatised splat (+ image
        reuse, on by default).  All three front-end contrast measures have an adjoint form (GRADIENT_MAGNITUDE: Sobel
        transposes in the image pass); an image with a side <= 2 * blur radius + 1 keeps the derivative-plane form."""
        self.set_grad_mode(_lib.GRAD_ADJOINT)
        self.set_splat_mode(1)

    def set_reference_path(self):
        """The reference's own data flow: derivative planes, one global fp32 atomic per vote (14-50x slower; also
        what produces the derivative images)."""
        self.set_grad_mode(_lib.GRAD_PLANES)
        self.set_splat_mode(0)

    def set_deterministic(self, on=True):
        """Bitwise run-to-run reproducible evaluations (CMX_OPT_DETERMINISTIC): integer vote accumulation in global
        memory, fixed summation orders everywhere; ~10-20 % slower.  Applies to the production path."""
        self.set_option(_lib.OPT_DETERMINISTIC, 1 if on else 0)

    def set_stream_priority(self, level):
        """cmx_set_stream_priority: > 0 highest (the front end beside a back-end solve), 0 normal, < 0 lowest."""
        self._ck(self._L.cmx_set_stream_priority(self._ctx, int(level)))

    def set_sched_class(self, sched_class):
        """cmx_set_sched_class: +1 urgent (the front end), 0 normal, -1 background (the back end: holds its next evaluation while an
        urgent context of the same device is busy)."""
        self._ck(self._L.cmx_set_sched_class(self._ctx, int(sched_class)))

    def set_cu_mask(self, n_cus=None, first=0, mask_words=None):
        """cmx_set_cu_mask: run on `n_cus` compute units starting at bit `first` (on MI355X consecutive bits walk the eight
        XCDs, so any run of bits is spread over all of them), or on an explicit list of 32-bit words; None / 0 = all."""
        if mask_words is None:
            if not n_cus:
                self._ck(self._L.cmx_set_cu_mask(self._ctx, None, 0))
                return
            bits = ((1 << int(n_cus)) - 1) << int(first)
            nw = max(8, (bits.bit_length() + 31) // 32)
            mask_words = [(bits >> (32 * i)) & 0xffffffff for i in range(nw)]
        arr = (C.c_uint32 * len(mask_words))(*mask_words)
        self._ck(self._L.cmx_set_cu_mask(self._ctx, arr, len(mask_words)))

    def set_stream(self, hip_stream_handle):
        """Run on a caller-owned stream (an int / void* hipStream_t, e.g. torch.cuda.current_stream().cuda_stream)."""
        self._ck(self._L.cmx_set_stream(self._ctx, C.c_void_p(hip_stream_handle or None)))

    # split-phase plumbing (multi-GPU): the accumulation planes between splat and blur/reduce
    def accum_capacity(self):
        return int(self._L.cmx_accum_capacity(self._ctx))

    def set_accum_buffer(self, device_ptr, n_floats):
        self._ck(self._L.cmx_set_accum_buffer(self._ctx, C.c_void_p(device_ptr), int(n_floats)))

    def accum_ptr(self):
        return self._L.cmx_accum_ptr(self._ctx)

    def accum_count(self):
        return int(self._L.cmx_accum_count(self._ctx))

    # native RCCL exchange inside the evaluator (one process per GPU)
    @staticmethod
    def comm_unique_id():
        buf = C.create_string_buffer(128)
        check(None, _lib.lib().cmx_comm_unique_id(buf))
        return buf.raw

    def comm_attach(self, unique_id, rank, nranks):
        self._ck(self._L.cmx_comm_attach(self._ctx, C.c_char_p(unique_id), int(rank), int(nranks)))

    def comm_attach_custom(self, fn, rank, nranks):
        """Exchange through a caller-supplied all-reduce: fn(device_ptr, count, dtype, op, hip_stream) -> 0 on success
        (dtype / op: _lib.DT_* / _lib.OP_*), called at the evaluator's exchange points in place of RCCL."""
        def tramp(_user, buf, count, dt, op, stream):
            try:
                return int(fn(buf, count, dt, op, stream) or 0)
            except Exception:  # an exception must not unwind through the C frames
                import traceback
                traceback.print_exc()
                return -1
        self._comm_cb = _lib.ALLREDUCE_FN(tramp)  # keep the trampoline alive as long as it is attached
        self._ck(self._L.cmx_comm_attach_custom(self._ctx, C.cast(self._comm_cb, C.c_void_p), None, int(rank), int(nranks)))

    def comm_detach(self):
        self._ck(self._L.cmx_comm_detach(self._ctx))

    def comm_info(self):
        """{'rank', 'nranks', 'transport'} as the attached communicator itself reports them (cmx_comm_info)."""
        r, n, t = C.c_int(), C.c_int(), C.c_int()
        self._ck(self._L.cmx_comm_info(self._ctx, C.byref(r), C.byref(n), C.byref(t)))
        return {"rank": r.value, "nranks": n.value, "transport": ("none", "rccl", "custom/direct")[t.value]}

    def set_grad_buffer(self, device_ptr, n_doubles):
        self._ck(self._L.cmx_set_grad_buffer(self._ctx, C.c_void_p(device_ptr), int(n_doubles)))

    def grad_count(self):
        return int(self._L.cmx_grad_count(self._ctx))

    def finish_begin(self, want_grad=True):
        fn = self._L.cmx_frontend_finish_begin if isinstance(self, FrontendEvaluator) else self._L.cmx_backend_finish_begin
        self._ck(fn(self._ctx, int(bool(want_grad))))

    def finish_end(self, want_grad=True):
        fe = isinstance(self, FrontendEvaluator)
        n = 3 if fe else self.num_params
        c = C.c_double()
        g = np.zeros(max(n, 1))
        fn = self._L.cmx_frontend_finish_end if fe else self._L.cmx_backend_finish_end
        self._ck(fn(self._ctx, C.byref(c), _dp(g) if want_grad else None))
        return c.value, (g[:n] if want_grad else None)

    def eval_many(self, xs, want_grad=True):
        """m independent evaluations in one call (cmx_*_eval_many): xs = m x n_params.  Returns (contrasts[m], grads[m, n] | None)."""
        fe = isinstance(self, FrontendEvaluator)
        n = 3 if fe else self.num_params
        xs = np.ascontiguousarray(np.asarray(xs, np.float64).reshape(-1, max(n, 1)))
        m = xs.shape[0]
        c = np.zeros(m)
        g = np.zeros((m, max(n, 1))) if want_grad else None
        fn = self._L.cmx_frontend_eval_many if fe else self._L.cmx_backend_eval_many
        self._ck(fn(self._ctx, m, _dp(xs), _dp(c), _dp(g) if want_grad else None))
        return c, (g[:, :n] if want_grad else None)

    def eval_each(self, xs, want_grad=True):
        """m evaluations one after the other inside ONE native call (cmx_*_eval_each): the same as [self.eval(x) for x in xs]
        without the interpreter between them.  Returns (contrasts[m], grads[m, n] | None)."""
        return self.prepare_eval_each(xs, want_grad)()

    def prepare_eval_each(self, xs, want_grad=True):
        """eval_each in two steps: everything the interpreter does around the native call (array conversion, output buffers, ctypes
        pointers: ~10 us) now, the call itself when the returned function is called -- for callers that time a short list."""
        fe = isinstance(self, FrontendEvaluator)
        n = 3 if fe else self.num_params
        xs = np.ascontiguousarray(np.asarray(xs, np.float64).reshape(-1, max(n, 1)))
        m = xs.shape[0]
        c = np.zeros(m)
        g = np.zeros((m, max(n, 1))) if want_grad else None
        fn = self._L.cmx_frontend_eval_each if fe else self._L.cmx_backend_eval_each
        ctx, px, pc, pg, ck = self._ctx, _dp(xs), _dp(c), (_dp(g) if want_grad else None), self._ck

        def call():
            ck(fn(ctx, m, px, pc, pg))
            return c, (g[:, :n] if want_grad else None)
        return call

    def timing_enable(self, on=True, every=1):
        """on: True = all kernel classes, False = off, or an iterable of class names (e.g. ["splat"]).
        every: sample every n-th evaluation only (the per-event kernels are timed through events attached to the
        kernel itself, which costs ~1.5 us per timed launch)."""
        if on is True:
            mask = (1 << _lib.T_COUNT) - 1
        elif not on:
            mask = 0
        else:
            mask = sum(1 << _lib.T_NAMES.index(n) for n in on)
        self._ck(self._L.cmx_timing_enable(self._ctx, mask | (int(every) << 8) if mask else 0))

    def timing_get(self):
        """{'splat': (ms, launches), ...} accumulated since the last call."""
        ms = np.zeros(_lib.T_COUNT)
        n = np.zeros(_lib.T_COUNT, np.int64)
        self._ck(self._L.cmx_timing_get(self._ctx, _dp(ms), n.ctypes.data_as(c_i64p)))
        return {name: (float(ms[i]), int(n[i])) for i, name in enumerate(_lib.T_NAMES)}


class EventStore:
    """Device-resident copy of the event stream (the reference's AngVelEstimator::events_): push chunks as they
    arrive, cut packets / windows from it by global event index, drop the prefix like deleteOldEvents."""

    def __init__(self, W, H, capacity, device=0, devices=None):
        """devices = [d0, d1, ...] (a group's member list): one replica of the stream on every distinct device
        (cmx_events_create_group); a group handle over the same list cuts its windows from it member by member."""
        self._L = _lib.lib()
        self._h = C.c_void_p()
        self.W, self.H = int(W), int(H)
        if devices is None:
            check(None, self._L.cmx_events_create(C.byref(self._h), int(device), int(W), int(H), int(capacity)))
        else:
            dv = (C.c_int * len(devices))(*[int(d) for d in devices])
            check(None, self._L.cmx_events_create_group(C.byref(self._h), dv, len(devices), int(W), int(H), int(capacity)))

    @property
    def devices(self):
        dv = (C.c_int * 16)()
        n = self._L.cmx_events_devices(self._h, dv, 16)
        return list(dv[:n])

    def _ck(self, status):
        if status != _lib.OK:
            raise CmaxHipError(status, self._L.cmx_status_string(status).decode() + ": " +
                               self._L.cmx_events_last_error(self._h).decode())

    def push(self, x, y, t_ns, polarity=None):
        """polarity (one value per event, nonzero = ON): cmx_events_push_pol -- the store keeps it for reconstruct_pol_add_from.
        A store holds polarity for all of its events or for none."""
        x, y, t = _c(x, np.uint16), _c(y, np.uint16), _c(t_ns, np.int64)
        if polarity is None:
            self._ck(self._L.cmx_events_push(self._h, len(x), x.ctypes.data_as(c_u16p), y.ctypes.data_as(c_u16p),
                                             t.ctypes.data_as(c_i64p)))
            return
        p = _pol_bytes(polarity)
        if not (len(x) == len(y) == len(t) == len(p)):
            raise ValueError("x, y, t_ns, polarity must have equal length")
        self._ck(self._L.cmx_events_push_pol(self._h, len(x), x.ctypes.data_as(c_u16p), y.ctypes.data_as(c_u16p),
                                             t.ctypes.data_as(c_i64p), p.ctypes.data_as(_lib.c_u8p)))

    def push_aos(self, events, polarity_field=None):
        """cmx_events_push_aos: records with fields x, y, sec, nsec (msg->events as it lies in the host's memory).
        polarity_field = the name of a one-byte field of the records (e.g. "polarity"): cmx_events_push_aos_pol."""
        ev = np.ascontiguousarray(events)
        lay = _lib.aos_layout_of(ev)
        if polarity_field is None:
            self._ck(self._L.cmx_events_push_aos(self._h, len(ev), ev.ctypes.data_as(C.c_void_p), C.byref(lay)))
        else:
            self._ck(self._L.cmx_events_push_aos_pol(self._h, len(ev), ev.ctypes.data_as(C.c_void_p), C.byref(lay),
                                                     _pol_offset(ev, polarity_field)))

    @property
    def has_polarity(self):
        return bool(self._L.cmx_events_has_polarity(self._h))

    def drop_before(self, global_index):
        self._ck(self._L.cmx_events_drop_before(self._h, int(global_index)))

    def select(self, src, first, count, keep=None, score=None, min_score=None, flags=None, flags_mask=3, flags_value=3,
               pixel_keep=None):
        """cmx_events_select*: append to THIS store the events of src[first, first+count) for which every given criterion holds, in
        their order (a stable compaction on the device); returns how many were kept.  keep: `count` bytes, nonzero = keep.  score with
        min_score: `count` float32, keep when score >= min_score (NaN is dropped).  flags: `count` bytes, keep when
        (flags & flags_mask) == flags_value -- the default 3 / 3 is "the event voted", the bit pair of reconstruct_warp / _score.
        pixel_keep: (H, W) bytes, nonzero = the pixel's events are kept.  No criterion: a device-side copy of the range.
        numpy arrays take the host form; objects with data_ptr() (torch tensors on the stores' device, contiguous: uint8 / bool, float32)
        the device form, in which nothing crosses the host.  The two kinds cannot be mixed."""
        first, count = int(first), int(count)
        if (score is None) != (min_score is None):
            raise ValueError("score and min_score are given together")
        given = [a for a in (keep, score, flags, pixel_keep) if a is not None]
        on_device = [hasattr(a, "data_ptr") for a in given]
        if any(on_device) and not all(on_device):
            raise ValueError("criteria are all host arrays or all device tensors")
        device = bool(on_device) and on_device[0]
        hold = []  # (the host arrays must outlive the call)

        def ptr(a, name, n, host_dtype, itemsize):
            if a is None:
                return None
            if device:
                _on_device(a, name)
                if int(a.numel()) != n or int(a.element_size()) != itemsize or not a.is_contiguous():
                    raise ValueError("%s: %d contiguous elements of %d byte(s) expected" % (name, n, itemsize))
                return a.data_ptr()
            a = np.asarray(a)
            if host_dtype == np.uint8 and a.dtype == np.bool_:
                a = a.view(np.uint8)
            a = _c(a, host_dtype).reshape(-1)
            if a.size != n:
                raise ValueError("%s: %d elements expected, got %d" % (name, n, a.size))
            hold.append(a)
            return a.ctypes.data

        sel = _lib.Select(C.sizeof(_lib.Select), ptr(keep, "keep", count, np.uint8, 1), ptr(score, "score", count, np.float32, 4),
                          float(min_score) if min_score is not None else 0.0, ptr(flags, "flags", count, np.uint8, 1),
                          int(flags_mask) & 255, int(flags_value) & 255, ptr(pixel_keep, "pixel_keep", self.W * self.H, np.uint8, 1))
        kept = C.c_int64(0)
        fn = self._L.cmx_events_select_device if device else self._L.cmx_events_select
        self._ck(fn(self._h, src._h, first, count, C.byref(sel), C.byref(kept)))
        return int(kept.value)

    def pixel_counts(self, first, count, out=None):
        """cmx_events_pixel_counts*: (H, W) uint32, the number of events of [first, first+count) at every pixel -- what a hot-pixel mask
        is made from.  out: a tensor of W*H 32-bit words on the store's device, filled and returned instead."""
        if out is not None:
            _on_device(out, "out")
            if int(out.numel()) != self.W * self.H or int(out.element_size()) != 4 or not out.is_contiguous():
                raise ValueError("out: W*H contiguous 32-bit elements expected")
            self._ck(self._L.cmx_events_pixel_counts_device(self._h, int(first), int(count), out.data_ptr()))
            return out
        counts = np.empty((self.H, self.W), np.uint32)
        self._ck(self._L.cmx_events_pixel_counts(self._h, int(first), int(count), counts.ctypes.data))
        return counts

    def read(self, first, count):
        """cmx_events_read: (x, y, t_ns, polarity or None) of [first, first+count), the inverse of push."""
        n = max(int(count), 0)
        x, y, t = np.empty(n, np.uint16), np.empty(n, np.uint16), np.empty(n, np.int64)
        p = np.empty(n, np.uint8) if self.has_polarity else None
        self._ck(self._L.cmx_events_read(self._h, int(first), int(count), x.ctypes.data_as(c_u16p), y.ctypes.data_as(c_u16p),
                                         t.ctypes.data_as(c_i64p), p.ctypes.data_as(_lib.c_u8p) if p is not None else None))
        return x, y, t, p

    @property
    def begin(self):
        return int(self._L.cmx_events_begin(self._h))

    @property
    def end(self):
        return int(self._L.cmx_events_end(self._h))

    def close(self):
        if getattr(self, "_h", None):
            self._L.cmx_events_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FrontendEvaluator(_Evaluator):
    def __init__(self, W, H, lut, device=0):
        super().__init__()
        self.W, self.H = int(W), int(H)
        lut = _c(lut, np.float64).reshape(-1)
        if lut.size != self.W * self.H * 3:
            raise ValueError("lut must hold W*H*3 doubles")
        self._ck(self._L.cmx_frontend_create(C.byref(self._ctx), int(device), self.W, self.H, _dp(lut)))
        self.n_events = 0

    def set_packet(self, x, y, t_ns, t_ref_ns, fx, fy, cx, cy, event_batch_size=100, blur_sigma=1.0,
                   contrast_measure=VARIANCE):
        x, y, t = _c(x, np.uint16), _c(y, np.uint16), _c(t_ns, np.int64)
        if not (len(x) == len(y) == len(t)):
            raise ValueError("x, y, t_ns must have equal length")
        self._ck(self._L.cmx_frontend_set_packet(
            self._ctx, len(x), x.ctypes.data_as(c_u16p), y.ctypes.data_as(c_u16p), t.ctypes.data_as(c_i64p),
            int(t_ref_ns), float(fx), float(fy), float(cx), float(cy), int(event_batch_size), float(blur_sigma),
            int(contrast_measure)))
        self.n_events = len(x)

    def set_packet_aos(self, events, t_ref_ns, fx, fy, cx, cy, event_batch_size=100, blur_sigma=1.0, contrast_measure=VARIANCE):
        """cmx_frontend_set_packet_aos: `events` = structured array of records with fields x, y, sec, nsec (e.g. _lib.DVS_EVENT_DTYPE)."""
        ev = np.ascontiguousarray(events)
        lay = _lib.aos_layout_of(ev)
        self._ck(self._L.cmx_frontend_set_packet_aos(self._ctx, len(ev), ev.ctypes.data_as(C.c_void_p), C.byref(lay), int(t_ref_ns),
                                                     float(fx), float(fy), float(cx), float(cy), int(event_batch_size),
                                                     float(blur_sigma), int(contrast_measure)))
        self.n_events = len(ev)

    def set_packet_from(self, store, first, count, t_ref_ns, fx, fy, cx, cy, event_batch_size=100, blur_sigma=1.0,
                        contrast_measure=VARIANCE):
        """The packet events_[first, first+count) cut from a device-resident EventStore (no host copy)."""
        self._ck(self._L.cmx_frontend_set_packet_from(self._ctx, store._h, int(first), int(count), int(t_ref_ns), float(fx),
                                                      float(fy), float(cx), float(cy), int(event_batch_size),
                                                      float(blur_sigma), int(contrast_measure)))
        self.n_events = int(count)

    def prepare(self, ang_vel_hint=(0.0, 0.0, 0.0)):
        """cmx_frontend_prepare: queue the packet's tile sort / streams / chunk table now (non-blocking); results never depend on
        the hint."""
        h = np.ascontiguousarray(ang_vel_hint, dtype=np.float64)
        self._ck(self._L.cmx_frontend_prepare(self._ctx, _dp(h)))

    def eval(self, ang_vel, want_grad=True):
        """(contrast, gradient[3] | None) -- what computeContrast returns."""
        self._io_buffers(3)
        self._xin[:] = ang_vel
        rc = self._L.cmx_frontend_eval(self._ctx, self._xp, self._cref, self._gp if want_grad else None)
        if rc:
            self._ck(rc)
        return self._cb.value, (self._gout.copy() if want_grad else None)

    def accumulate(self, ang_vel, want_grad=True):
        om = _c(ang_vel, np.float64)
        self._ck(self._L.cmx_frontend_accumulate(self._ctx, _dp(om), int(bool(want_grad))))

    def finish(self, want_grad=True):
        c = C.c_double()
        g = np.zeros(3)
        self._ck(self._L.cmx_frontend_finish(self._ctx, C.byref(c), _dp(g) if want_grad else None))
        return c.value, (g if want_grad else None)

    def adjoint_plane(self):
        """Diagnostic (cmx_diag_get_adjoint_plane): Jt, (H, W) fp32, as the last adjoint image pass left it -- tiles that pass
        skipped keep older values."""
        return self._adjoint_plane(_lib.DIAG_JT_EVAL, self.H, self.W)

    def forward_plane(self):
        """Diagnostic (cmx_diag_get_forward_plane): the forward plane before the blur, (H, W) fp32 -- the votes of the context's last
        splat, whichever call made it (an evaluation's fused splat included); nothing is launched."""
        out = np.empty((self.H, self.W), np.float32)
        self._ck(self._L.cmx_diag_get_forward_plane(self._ctx, out.ctypes.data_as(c_fp)))
        return out

    # --- reference-named entry points
    def computeImageOfWarpedEvents(self, ang_vel, want_deriv=False, blur=True):
        """image_warped (H x W fp32) [, image_warped_deriv (H x W x 3 fp32)]."""
        om = _c(ang_vel, np.float64)
        iwe = np.empty((self.H, self.W), np.float32)
        d = np.empty((self.H, self.W, 3), np.float32) if want_deriv else None
        self._ck(self._L.cmx_frontend_get_iwe(self._ctx, _dp(om), int(bool(blur)), iwe.ctypes.data_as(c_fp),
                                              d.ctypes.data_as(c_fp) if want_deriv else None))
        return (iwe, d) if want_deriv else iwe

    def publishEventImage(self, ang_vel):
        """AngVelEstimator::publishEventImage: (H, 2W) uint8, raw events left, motion-compensated at `ang_vel` right,
        one common range, dark events on white.  Tone-mapped on the device."""
        om = _c(ang_vel, np.float64)
        out = np.empty((self.H, 2 * self.W), np.uint8)
        self._ck(self._L.cmx_frontend_render_display(self._ctx, _dp(om), out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def contrast_fdf(self, v):
        c, g = self.eval(v, True)
        return -c, -g

    def contrast_f(self, v):
        return -self.eval(v, False)[0]

    def contrast_df(self, v):
        return -self.eval(v, True)[1]

    def setupProblemAndOptimize(self, ang_vel):
        """FR-CG solve from the warm start `ang_vel` (local_optim_contrast_gsl.cpp:74-233).
        Returns (ang_vel_estimate, report dict)."""
        x = np.array(ang_vel, dtype=np.float64, order="C", copy=True)
        rep = _lib.SolveReport()
        self._ck(self._L.cmx_frontend_solve(self._ctx, _dp(x), C.byref(rep)))
        return x, {f: getattr(rep, f) for f, _ in rep._fields_}


class BackendEvaluator(_Evaluator):
    def __init__(self, W, H, lut, pano_width, pano_height, device=0, devices=None, transport=0):
        """devices = [d0, d1, ...]: a one-process multi-GPU GROUP (cmx_backend_create_group) behind the same interface --
        set_window shards the window, eval / setupProblemAndOptimize fan out and return one contrast / gradient.  The same
        device may be listed more than once (members sharing a GPU: how a one-GPU box exercises the group)."""
        super().__init__()
        self.W, self.H, self.Wp, self.Hp = int(W), int(H), int(pano_width), int(pano_height)
        lut = _c(lut, np.float64).reshape(-1)
        if lut.size != self.W * self.H * 3:
            raise ValueError("lut must hold W*H*3 doubles")
        if devices is None:
            self._ck(self._L.cmx_backend_create(C.byref(self._ctx), int(device), self.W, self.H, _dp(lut), self.Wp, self.Hp))
        else:
            dv = (C.c_int * len(devices))(*[int(d) for d in devices])
            self._ck(self._L.cmx_backend_create_group(C.byref(self._ctx), dv, len(devices), self.W, self.H, _dp(lut), self.Wp,
                                                      self.Hp, int(transport)))
        self.K = self.num_fixed = 0

    def group_info(self):
        """{'members', 'devices', 'transport', 'events_per_member', 'last_fanout_us'} of this handle (a plain context: 1 member)."""
        n, tr, us = C.c_int(), C.c_int(), C.c_double()
        dev = (C.c_int * 16)()
        ev = np.zeros(16, np.int64)
        self._ck(self._L.cmx_group_info(self._ctx, C.byref(n), dev, 16, C.byref(tr), ev.ctypes.data_as(c_i64p), C.byref(us)))
        return {"members": n.value, "devices": list(dev[:n.value]), "transport": tr.value,
                "events_per_member": [int(v) for v in ev[:n.value]], "last_fanout_us": us.value}

    def group_transport_info(self):
        """{'chosen', 'measured', 'us_direct', 'us_rccl'}: cmx_group_transport_info (CMX_GROUP_AUTO times the candidates at creation)."""
        ch, me, ud, ur = C.c_int(), C.c_int(), C.c_double(), C.c_double()
        self._ck(self._L.cmx_group_transport_info(self._ctx, C.byref(ch), C.byref(me), C.byref(ud), C.byref(ur)))
        return {"chosen": ch.value, "measured": bool(me.value), "us_direct": ud.value, "us_rccl": ur.value}

    def get_pose_table(self):
        """cmx_backend_get_pose_table: (R[nb,3,3] fp64, Jcp[nb,3,3*order] fp32, idx[nb], t_batch_ns[nb]) at the last evaluation's
        parameters -- what Trajectory::evaluate returns per batch (value, ddrot_ddrot_cp, idx_cp_beg)."""
        nb = C.c_int()
        self._ck(self._L.cmx_backend_get_pose_table(self._ctx, 0, None, None, None, None, C.byref(nb)))
        n = nb.value
        R = np.zeros((max(n, 1), 9))
        J = np.zeros((max(n, 1), 36), np.float32)
        idx = np.zeros(max(n, 1), np.int32)
        t = np.zeros(max(n, 1), np.int64)
        self._ck(self._L.cmx_backend_get_pose_table(self._ctx, n, _dp(R), J.ctypes.data_as(c_fp), idx.ctypes.data_as(C.POINTER(C.c_int)),
                                                    t.ctypes.data_as(c_i64p), C.byref(nb)))
        order = self._order
        return (R[:n].reshape(n, 3, 3), J[:n, :9 * order].reshape(n, 3, 3 * order), idx[:n].copy(), t[:n].copy())

    @property
    def num_params(self):
        return 3 * (self.K - self.num_fixed)

    def set_window(self, x, y, t_ns, order, knots_xyzw, start_ns, dt_ns, num_fixed, t_next_win_beg_ns,
                   event_batch_size=100, event_sample_rate=1, blur_sigma=1.0, contrast_measure=VARIANCE, IG=None):
        x, y, t = _c(x, np.uint16), _c(y, np.uint16), _c(t_ns, np.int64)
        if not (len(x) == len(y) == len(t)):
            raise ValueError("x, y, t_ns must have equal length")
        k = _c(knots_xyzw, np.float64).reshape(-1, 4)
        ig = None
        keep = isinstance(IG, str) and IG == "resident"  # CMX_KEEP_MAP: use the device-resident global map
        if IG is not None and not keep:
            ig = _c(IG, np.float32)
            if ig.size != self.Wp * self.Hp:
                raise ValueError("IG must be Hp x Wp")
        self._ck(self._L.cmx_backend_set_window(
            self._ctx, len(x), x.ctypes.data_as(c_u16p), y.ctypes.data_as(c_u16p), t.ctypes.data_as(c_i64p),
            int(order), k.shape[0], _dp(k), int(start_ns), int(dt_ns), int(num_fixed), int(t_next_win_beg_ns),
            int(event_batch_size), int(event_sample_rate), float(blur_sigma), int(contrast_measure),
            C.cast(C.c_void_p(1), c_fp) if keep else (ig.ctypes.data_as(c_fp) if ig is not None else None)))
        self.K, self.num_fixed, self._order = k.shape[0], int(num_fixed), int(order)

    def set_window_aos(self, events, order, knots_xyzw, start_ns, dt_ns, num_fixed, t_next_win_beg_ns, event_batch_size=100,
                       event_sample_rate=1, blur_sigma=1.0, contrast_measure=VARIANCE, IG=None):
        """cmx_backend_set_window_aos: `events` = structured array of records with fields x, y, sec, nsec."""
        ev = np.ascontiguousarray(events)
        lay = _lib.aos_layout_of(ev)
        k = _c(knots_xyzw, np.float64).reshape(-1, 4)
        keep = isinstance(IG, str) and IG == "resident"
        ig = _c(IG, np.float32) if (IG is not None and not keep) else None
        self._ck(self._L.cmx_backend_set_window_aos(
            self._ctx, len(ev), ev.ctypes.data_as(C.c_void_p), C.byref(lay), int(order), k.shape[0], _dp(k), int(start_ns), int(dt_ns),
            int(num_fixed), int(t_next_win_beg_ns), int(event_batch_size), int(event_sample_rate), float(blur_sigma), int(contrast_measure),
            C.cast(C.c_void_p(1), c_fp) if keep else (ig.ctypes.data_as(c_fp) if ig is not None else None)))
        self.K, self.num_fixed, self._order = k.shape[0], int(num_fixed), int(order)

    def set_window_from(self, store, first, count, order, knots_xyzw, start_ns, dt_ns, num_fixed, t_next_win_beg_ns,
                        event_batch_size=100, event_sample_rate=1, blur_sigma=1.0, contrast_measure=VARIANCE, IG=None):
        """The window events_[first, first+count) cut from a device-resident EventStore."""
        k = _c(knots_xyzw, np.float64).reshape(-1, 4)
        keep = isinstance(IG, str) and IG == "resident"
        ig = _c(IG, np.float32) if (IG is not None and not keep) else None
        self._ck(self._L.cmx_backend_set_window_from(
            self._ctx, store._h, int(first), int(count), int(order), k.shape[0], _dp(k), int(start_ns), int(dt_ns),
            int(num_fixed), int(t_next_win_beg_ns), int(event_batch_size), int(event_sample_rate), float(blur_sigma),
            int(contrast_measure),
            C.cast(C.c_void_p(1), c_fp) if keep else (ig.ctypes.data_as(c_fp) if ig is not None else None)))
        self.K, self.num_fixed, self._order = k.shape[0], int(num_fixed), int(order)

    def prepare(self, drotv_hint=None):
        """cmx_backend_prepare: pose table at the hint, tile sort, chunk table and bearing streams of the window, queued now."""
        h = None if drotv_hint is None else np.ascontiguousarray(drotv_hint, dtype=np.float64)
        self._ck(self._L.cmx_backend_prepare(self._ctx, _dp(h) if h is not None else None))

    def eval(self, drotv, want_grad=True):
        P = self.num_params
        if np.size(drotv) != P:
            raise ValueError("drotv must hold 3*(K-num_fixed) doubles")
        self._io_buffers(P)
        if P:
            self._xin[:P] = np.reshape(drotv, -1)
        rc = self._L.cmx_backend_eval(self._ctx, self._xp, self._cref, self._gp if want_grad else None)
        if rc:
            self._ck(rc)
        return self._cb.value, (self._gout[:P].copy() if want_grad else None)

    def accumulate(self, drotv, want_grad=True):
        d = _c(drotv, np.float64).reshape(-1)
        self._ck(self._L.cmx_backend_accumulate(self._ctx, _dp(d), int(bool(want_grad))))

    def finish(self, want_grad=True):
        c = C.c_double()
        g = np.zeros(max(self.num_params, 1))
        self._ck(self._L.cmx_backend_finish(self._ctx, C.byref(c), _dp(g) if want_grad else None))
        return c.value, (g[:self.num_params] if want_grad else None)

    def get_plane(self, which):
        out = np.empty((self.Hp, self.Wp), np.float32)
        self._ck(self._L.cmx_backend_get_plane(self._ctx, int(which), out.ctypes.data_as(c_fp)))
        return out

    def adjoint_plane(self):
        """Diagnostic (cmx_diag_get_adjoint_plane): the window's Jt, (Hp, Wp) fp32, as the last adjoint image pass left it --
        tiles that pass skipped keep older values."""
        return self._adjoint_plane(_lib.DIAG_JT_EVAL, self.Hp, self.Wp)

    def reconstruct_adjoint_plane(self):
        """... and the whole-trajectory reconstruction's Jt (its own plane, not the window's)."""
        return self._adjoint_plane(_lib.DIAG_JT_RECON, self.Hp, self.Wp)

    @property
    def alpha(self):
        a = C.c_double()
        self._ck(self._L.cmx_backend_get_alpha(self._ctx, C.byref(a)))
        return a.value

    # --- global-map upkeep (EventWarper::updateIG / setUpdateTimesIG / resetIG), device-resident
    def updateIG(self, max_update_times):
        self._ck(self._L.cmx_backend_update_map(self._ctx, int(max_update_times)))

    def setUpdateTimesIG(self, quat_xyzw, radius=3):
        q = _c(quat_xyzw, np.float64)
        self._ck(self._L.cmx_backend_mark_visited(self._ctx, _dp(q), int(radius)))

    def resetIG(self):
        self._ck(self._L.cmx_backend_reset_map(self._ctx))

    def getIG(self, with_visits=False):
        ig = np.empty((self.Hp, self.Wp), np.float32)
        v = np.empty((self.Hp, self.Wp), np.uint8) if with_visits else None
        self._ck(self._L.cmx_backend_get_map(self._ctx, ig.ctypes.data_as(c_fp),
                                             v.ctypes.data_as(C.POINTER(C.c_uint8)) if with_visits else None))
        return (ig, v) if with_visits else ig

    def publishEventImage(self, gamma=0.75, fov_quat=None):
        """PoseGraphOptimizer::publishEventImage on the resident map: (Hp, Wp) uint8, or (Hp, Wp, 3) BGR uint8 with the
        sensor outline at pose `fov_quat` (xyzw) drawn in (255, 0, 0).  Tone-mapped on the device."""
        q = _c(fov_quat, np.float64) if fov_quat is not None else None
        out = np.empty((self.Hp, self.Wp) if q is None else (self.Hp, self.Wp, 3), np.uint8)
        self._ck(self._L.cmx_backend_render_map(self._ctx, float(gamma), _dp(q) if q is not None else None,
                                                out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def setIG(self, IG=None, visits=None):
        ig = _c(IG, np.float32) if IG is not None else None
        v = _c(visits, np.uint8) if visits is not None else None
        self._ck(self._L.cmx_backend_set_map(self._ctx, ig.ctypes.data_as(c_fp) if ig is not None else None,
                                             v.ctypes.data_as(C.POINTER(C.c_uint8)) if v is not None else None))

    # --- whole-trajectory reconstruction (cmx_backend_recon_*): all events along the final spline, any knot count
    _recon_K = 0  # knots of the last reconstruct_begin (0: none yet -- the library reports the state error)

    def reconstruct_begin(self, order, knots_xyzw, start_ns, dt_ns, event_batch_size=100, event_sample_rate=1):
        """Start a reconstruction along the spline (order 2 | 4, K >= order knots, no upper bound on K): zeroes a plane that
        belongs to the reconstruction alone and records the current deterministic setting.  A second call starts over."""
        k = _c(knots_xyzw, np.float64).reshape(-1, 4)
        self._recon_K = k.shape[0]
        self._view_shape = None  # (begin frees a view set)
        self._voxel_shape = None  # (... and a voxel set)
        self._surface_shape = None  # (... and a surface set)
        self._ck(self._L.cmx_backend_recon_begin(self._ctx, int(order), k.shape[0], _dp(k), int(start_ns), int(dt_ns),
                                                 int(event_batch_size), int(event_sample_rate)))

    def reconstruct_add(self, x, y, t_ns):
        """One vote loop over exactly these events (batches start at the first one), added to the plane."""
        x, y, t = _c(x, np.uint16), _c(y, np.uint16), _c(t_ns, np.int64)
        if not (len(x) == len(y) == len(t)):
            raise ValueError("x, y, t_ns must have equal length")
        self._ck(self._L.cmx_backend_recon_add(self._ctx, len(x), x.ctypes.data_as(c_u16p), y.ctypes.data_as(c_u16p),
                                               t.ctypes.data_as(c_i64p)))

    def reconstruct_add_aos(self, events):
        """The same from a structured array of records with fields x, y, sec, nsec (e.g. _lib.DVS_EVENT_DTYPE)."""
        ev = np.ascontiguousarray(events)
        lay = _lib.aos_layout_of(ev)
        self._ck(self._L.cmx_backend_recon_add_aos(self._ctx, len(ev), ev.ctypes.data_as(C.c_void_p), C.byref(lay)))

    def reconstruct_add_from(self, store, first, count):
        """The same over events_[first, first+count) of a device-resident EventStore (nothing crosses the host)."""
        self._ck(self._L.cmx_backend_recon_add_from(self._ctx, store._h, int(first), int(count)))

    # --- per-event export: where every event lands under the knots the reconstruction holds now (cmx_backend_recon_warp*)
    @staticmethod
    def _warp_out(n, dtype):
        dt = np.dtype(dtype)
        if dt not in (np.dtype(np.float64), np.dtype(np.float32)):
            raise ValueError("dtype must be float64 or float32")
        return (_lib.WARP_F64 if dt == np.dtype(np.float64) else _lib.WARP_F32), np.empty((n, 2), dt), np.empty(n, np.uint8)

    def reconstruct_warp(self, x, y, t_ns, dtype=np.float64):
        """(xy[n, 2], flags[n] uint8) of exactly these events, sampled or not, in input order: the panorama coordinate the vote
        kernels take cell and weights from, and flags = WARP_SAMPLED | WARP_INSIDE (3: the event votes in reconstruct_add).
        Reads the knots only; changes nothing."""
        x, y, t = _c(x, np.uint16), _c(y, np.uint16), _c(t_ns, np.int64)
        if not (len(x) == len(y) == len(t)):
            raise ValueError("x, y, t_ns must have equal length")
        fmt, xy, fl = self._warp_out(len(x), dtype)
        self._ck(self._L.cmx_backend_recon_warp(self._ctx, len(x), x.ctypes.data_as(c_u16p), y.ctypes.data_as(c_u16p),
                                                t.ctypes.data_as(c_i64p), fmt, xy.ctypes.data, fl.ctypes.data))
        return xy, fl

    def reconstruct_warp_aos(self, events, dtype=np.float64):
        """The same from a structured array of records with fields x, y, sec, nsec."""
        ev = np.ascontiguousarray(events)
        lay = _lib.aos_layout_of(ev)
        fmt, xy, fl = self._warp_out(len(ev), dtype)
        self._ck(self._L.cmx_backend_recon_warp_aos(self._ctx, len(ev), ev.ctypes.data_as(C.c_void_p), C.byref(lay), fmt,
                                                    xy.ctypes.data, fl.ctypes.data))
        return xy, fl

    def reconstruct_warp_from(self, store, first, count, dtype=np.float64, out=None):
        """The same over events_[first, first+count) of an EventStore.  out = (xy, flags), objects with data_ptr() (torch tensors on
        the context's device: xy of `count` x 2 elements of dtype, flags of `count` bytes or None): the kernel writes straight into
        them, nothing crosses the host, and out is returned.  The call runs on the context's stream and returns when the outputs are
        complete; work of the caller's that still writes the tensors on another stream must be finished before it."""
        if out is not None:
            xy, fl = out
            fmt = self._warp_out(0, dtype)[0]
            self._ck(self._L.cmx_backend_recon_warp_from_device(self._ctx, store._h, int(first), int(count), fmt, xy.data_ptr(),
                                                                fl.data_ptr() if fl is not None else None))
            return out
        fmt, xy, fl = self._warp_out(int(count), dtype)
        self._ck(self._L.cmx_backend_recon_warp_from(self._ctx, store._h, int(first), int(count), fmt, xy.ctypes.data, fl.ctypes.data))
        return xy, fl

    # --- per-event support scores: the panorama read back at every event (cmx_backend_recon_score*)
    def reconstruct_score_open(self, sigma=0.0):
        """Open a score pass: S = GaussianBlur(plane, sigma) of the plane as accumulated now (sigma 0: the plane itself).  It stays
        open until something changes the plane or the knots (add, restart, extend, eval, solve, bind, freeze / advance_head)."""
        self._ck(self._L.cmx_backend_recon_score_open(self._ctx, float(sigma)))

    def reconstruct_score_plane(self):
        """S of the open score pass, (Hp, Wp) float32."""
        S = np.empty((self.Hp, self.Wp), np.float32)
        self._ck(self._L.cmx_backend_recon_score_plane(self._ctx, S.ctypes.data_as(c_fp)))
        return S

    def reconstruct_score(self, x, y, t_ns, loo=True):
        """(scores float32[n], flags uint8[n]) of exactly these events, in input order: S interpolated with the vote's own four
        weights where the event lands (0 outside the plane), flags as reconstruct_warp.  loo: events that voted (flags == 3) have
        their own contribution subtracted; no clamp at zero.  Reads only."""
        x, y, t = _c(x, np.uint16), _c(y, np.uint16), _c(t_ns, np.int64)
        if not (len(x) == len(y) == len(t)):
            raise ValueError("x, y, t_ns must have equal length")
        sc, fl = np.empty(len(x), np.float32), np.empty(len(x), np.uint8)
        self._ck(self._L.cmx_backend_recon_score(self._ctx, len(x), x.ctypes.data_as(c_u16p), y.ctypes.data_as(c_u16p),
                                                 t.ctypes.data_as(c_i64p), int(bool(loo)), sc.ctypes.data, fl.ctypes.data))
        return sc, fl

    def reconstruct_score_aos(self, events, loo=True):
        """The same from a structured array of records with fields x, y, sec, nsec."""
        ev = np.ascontiguousarray(events)
        lay = _lib.aos_layout_of(ev)
        sc, fl = np.empty(len(ev), np.float32), np.empty(len(ev), np.uint8)
        self._ck(self._L.cmx_backend_recon_score_aos(self._ctx, len(ev), ev.ctypes.data_as(C.c_void_p), C.byref(lay), int(bool(loo)),
                                                     sc.ctypes.data, fl.ctypes.data))
        return sc, fl

    def reconstruct_score_from(self, store, first, count, loo=True, out=None):
        """The same over events_[first, first+count) of an EventStore.  out = (scores, flags_or_None), torch tensors on the context's
        device (`count` float32, `count` bytes): the kernel writes straight into them, nothing crosses the host, and out is returned
        (the stream rules of reconstruct_warp_from)."""
        if out is not None:
            sc, fl = out
            self._ck(self._L.cmx_backend_recon_score_from_device(self._ctx, store._h, int(first), int(count), int(bool(loo)), sc.data_ptr(),
                                                                 fl.data_ptr() if fl is not None else None))
            return out
        sc, fl = np.empty(int(count), np.float32), np.empty(int(count), np.uint8)
        self._ck(self._L.cmx_backend_recon_score_from(self._ctx, store._h, int(first), int(count), int(bool(loo)), sc.ctypes.data,
                                                      fl.ctypes.data))
        return sc, fl

    # --- signed polarity map: ON / OFF planes of the same vote loop (cmx_backend_recon_pol_*)
    def reconstruct_pol_add(self, x, y, t_ns, polarity):
        """reconstruct_add's vote loop over exactly these events, into the ON plane (polarity nonzero) or the OFF plane.  The count
        plane, its counters and every other state of the reconstruction are left alone."""
        x, y, t, p = _c(x, np.uint16), _c(y, np.uint16), _c(t_ns, np.int64), _pol_bytes(polarity)
        if not (len(x) == len(y) == len(t) == len(p)):
            raise ValueError("x, y, t_ns, polarity must have equal length")
        self._ck(self._L.cmx_backend_recon_pol_add(self._ctx, len(x), x.ctypes.data_as(c_u16p), y.ctypes.data_as(c_u16p),
                                                   t.ctypes.data_as(c_i64p), p.ctypes.data_as(_lib.c_u8p)))

    def reconstruct_pol_add_aos(self, events, polarity_field="polarity"):
        """The same from a structured array of records with fields x, y, sec, nsec and a one-byte polarity field."""
        ev = np.ascontiguousarray(events)
        lay = _lib.aos_layout_of(ev)
        self._ck(self._L.cmx_backend_recon_pol_add_aos(self._ctx, len(ev), ev.ctypes.data_as(C.c_void_p), C.byref(lay),
                                                       _pol_offset(ev, polarity_field)))

    def reconstruct_pol_add_from(self, store, first, count):
        """The same over events_[first, first+count) of an EventStore that holds polarity (EventStore.push(..., polarity=))."""
        self._ck(self._L.cmx_backend_recon_pol_add_from(self._ctx, store._h, int(first), int(count)))

    def reconstruct_pol_get(self, with_counts=False):
        """(on, off) -- two (Hp, Wp) fp32 planes [, events that voted ON, events that voted OFF]."""
        on, off = np.empty((self.Hp, self.Wp), np.float32), np.empty((self.Hp, self.Wp), np.float32)
        n_on, n_off = C.c_int64(), C.c_int64()
        self._ck(self._L.cmx_backend_recon_pol_get(self._ctx, on.ctypes.data_as(c_fp), off.ctypes.data_as(c_fp),
                                                   C.byref(n_on) if with_counts else None, C.byref(n_off) if with_counts else None))
        return (on, off, n_on.value, n_off.value) if with_counts else (on, off)

    def reconstruct_pol_render(self, gamma=0.75, mode=0):
        """The signed map ON - OFF tone-mapped on the device: mode 0 (POL_MONO8) -> (Hp, Wp) uint8, OFF dark / ON bright / 128
        where nothing voted; mode 1 (POL_BGR8) -> (Hp, Wp, 3) BGR on white, ON red, OFF blue."""
        out = np.empty((self.Hp, self.Wp, 3) if int(mode) == _lib.POL_BGR8 else (self.Hp, self.Wp), np.uint8)
        self._ck(self._L.cmx_backend_recon_pol_render(self._ctx, float(gamma), int(mode), out.ctypes.data_as(_lib.c_u8p)))
        return out

    def reconstruct_pol_reset(self):
        """Clear the ON / OFF planes and their counters (after the knots have moved); nothing else changes."""
        self._ck(self._L.cmx_backend_recon_pol_reset(self._ctx))

    # --- target sets: what the view, voxel and surface calls below share
    @staticmethod
    def _set_targets(targets):
        """(n, the ReconView array of a *_begin call) from _lib.ReconView structures or the tuples _lib.recon_view takes."""
        vs = [v if isinstance(v, _lib.ReconView) else _lib.recon_view(*v) for v in targets]
        return len(vs), (_lib.ReconView * max(len(vs), 1))(*vs)

    def _set_add(self, fn, x, y, t_ns, *pol):
        """fn(ctx, n, x, y, t_ns[, polarity]).  pol = (polarity, whether the set reads it) for the calls that take one."""
        x, y, t = _c(x, np.uint16), _c(y, np.uint16), _c(t_ns, np.int64)
        p = _pol_bytes(pol[0]) if pol and pol[0] is not None and pol[1] else None
        if not (len(x) == len(y) == len(t)) or (p is not None and len(p) != len(x)):
            raise ValueError("x, y, t_ns%s must have equal length" % (", polarity" if pol else ""))
        tail = (p.ctypes.data_as(_lib.c_u8p) if p is not None else None,) if pol else ()
        self._ck(fn(self._ctx, len(x), x.ctypes.data_as(c_u16p), y.ctypes.data_as(c_u16p), t.ctypes.data_as(c_i64p), *tail))

    def _set_add_aos(self, fn, events, *pol):
        """fn(ctx, n, records, layout[, polarity offset]).  pol = (polarity field, whether the set reads it)."""
        ev = np.ascontiguousarray(events)
        lay = _lib.aos_layout_of(ev)
        tail = (_pol_offset(ev, pol[0]) if pol[1] else 0,) if pol else ()
        self._ck(fn(self._ctx, len(ev), ev.ctypes.data_as(C.c_void_p), C.byref(lay), *tail))

    @staticmethod
    def _set_range(shape, first, count):
        """(count, the array shape of targets [first, first+count)) of a set of `shape` = (n, ...); count None: all from first."""
        count = shape[0] - int(first) if count is None else int(count)
        return count, (max(count, 0),) + tuple(shape[1:])

    def _set_get(self, shape, dtype, get, get_device, first, count, with_counts, out):
        """get(ctx, first, count, array | None, counters | None) into a new array of dtype, or get_device(ctx, first, count, pointer)
        into out; with_counts: (that, the int64 events that voted into each target)."""
        count, shape = self._set_range(shape, first, count)
        cnt = np.zeros(shape[0], np.int64)
        cnt_p = cnt.ctypes.data_as(c_i64p) if with_counts else None
        if out is not None:
            self._ck(get_device(self._ctx, int(first), count, out.data_ptr()))
            if with_counts:
                self._ck(get(self._ctx, int(first), count, None, cnt_p))
            return (out, cnt) if with_counts else out
        res = np.empty(shape, dtype)
        self._ck(get(self._ctx, int(first), count, res.ctypes.data_as(c_fp if dtype == np.float32 else c_i64p), cnt_p))
        return (res, cnt) if with_counts else res

    # --- pinhole views: motion-compensated frames and crops of the same vote loop (cmx_backend_recon_view_*)
    _view_shape = None  # (n_views, Hv, Wv) of the last reconstruct_view_begin

    def reconstruct_view_begin(self, views, Wv, Hv):
        """Attach virtual pinhole cameras to the open reconstruction and zero their (Hv, Wv) planes.  views: _lib.ReconView
        structures, or tuples (quat_xyzw, fx, fy, cx, cy, t_lo_ns, t_hi_ns) -- see trajectory.frame_views / crop_view."""
        n, arr = self._set_targets(views)
        self._view_shape = None
        self._ck(self._L.cmx_backend_recon_view_begin(self._ctx, int(Wv), int(Hv), n, arr))
        self._view_shape = (n, int(Hv), int(Wv))

    def reconstruct_view_add(self, x, y, t_ns):
        """reconstruct_add's vote loop over exactly these events: every sampled event is warped once into the world frame and
        voted into every view whose time range holds its batch time.  Nothing else of the reconstruction is read or written."""
        self._set_add(self._L.cmx_backend_recon_view_add, x, y, t_ns)

    def reconstruct_view_add_aos(self, events):
        """The same from a structured array of records with fields x, y, sec, nsec."""
        self._set_add_aos(self._L.cmx_backend_recon_view_add_aos, events)

    def reconstruct_view_add_from(self, store, first, count):
        """The same over events_[first, first+count) of a device-resident EventStore."""
        self._ck(self._L.cmx_backend_recon_view_add_from(self._ctx, store._h, int(first), int(count)))

    def reconstruct_view_get(self, first=0, count=None, with_counts=False):
        """(count, Hv, Wv) fp32 planes of views [first, first+count) [, int64 events that voted into each]."""
        return self._set_get(self._view_shape or (0, 0, 0), np.float32, self._L.cmx_backend_recon_view_get, None, first, count,
                             with_counts, None)

    def reconstruct_view_render(self, view, gamma=0.75):
        """reconstruct_render's tone map (no outline) on one view's plane: (Hv, Wv) uint8."""
        _, Hv, Wv = self._view_shape or (0, 0, 0)
        out = np.empty((Hv, Wv), np.uint8)
        self._ck(self._L.cmx_backend_recon_view_render(self._ctx, int(view), float(gamma), out.ctypes.data_as(_lib.c_u8p)))
        return out

    def reconstruct_view_reset(self):
        """Clear the view planes and their counters (after the knots have moved); the views stay."""
        self._ck(self._L.cmx_backend_recon_view_reset(self._ctx))

    def reconstruct_view_end(self):
        self._ck(self._L.cmx_backend_recon_view_end(self._ctx))
        self._view_shape = None

    # --- voxel grids: the discretised, polarity-signed event volume of the same vote loop (cmx_backend_recon_voxel_*)
    _voxel_shape = None  # (n_grids, n_bins, Hv, Wv) of the last reconstruct_voxel_begin
    _voxel_signed = True

    def reconstruct_voxel_begin(self, grids, Wv, Hv, n_bins, signed=True):
        """Attach voxel grids to the open reconstruction and zero their (n_bins, Hv, Wv) volumes.  grids: _lib.ReconView structures
        or tuples (quat_xyzw, fx, fy, cx, cy, t_lo_ns, t_hi_ns) with a finite time range -- see trajectory.voxel_grids.  signed:
        OFF events vote -1; otherwise every event votes +1 and polarity is never read."""
        n, arr = self._set_targets(grids)
        self._voxel_shape = None
        self._ck(self._L.cmx_backend_recon_voxel_begin(self._ctx, int(Wv), int(Hv), int(n_bins), int(bool(signed)), n, arr))
        self._voxel_shape = (n, int(n_bins), int(Hv), int(Wv))
        self._voxel_signed = bool(signed)

    def reconstruct_voxel_add(self, x, y, t_ns, polarity=None):
        """reconstruct_add's vote loop over exactly these events: every sampled event is warped once into the world frame and
        voted, by its OWN timestamp, into the two neighbouring bins of every grid whose range holds it.  polarity (one value per
        event, nonzero / positive = ON) is needed for a signed set and ignored by an unsigned one."""
        self._set_add(self._L.cmx_backend_recon_voxel_add, x, y, t_ns, polarity, self._voxel_signed)

    def reconstruct_voxel_add_aos(self, events, polarity_field="polarity"):
        """The same from a structured array of records with fields x, y, sec, nsec and a one-byte polarity field."""
        self._set_add_aos(self._L.cmx_backend_recon_voxel_add_aos, events, polarity_field, self._voxel_signed)

    def reconstruct_voxel_add_from(self, store, first, count):
        """The same over events_[first, first+count) of an EventStore (with polarity, EventStore.push(..., polarity=), for a
        signed set)."""
        self._ck(self._L.cmx_backend_recon_voxel_add_from(self._ctx, store._h, int(first), int(count)))

    def reconstruct_voxel_get(self, first=0, count=None, with_counts=False, out=None):
        """(count, n_bins, Hv, Wv) fp32 volumes of grids [first, first+count) [, int64 events that voted into each].  out: an object
        with data_ptr() -- a contiguous float32 torch tensor of that many elements on the context's device: the volumes are written
        straight into it, nothing crosses the host, and out is returned in the array's place.  The call runs on the context's stream
        and returns when out is complete; work of the caller's that still writes the tensor on another stream must be finished."""
        return self._set_get(self._voxel_shape or (0, 0, 0, 0), np.float32, self._L.cmx_backend_recon_voxel_get,
                             self._L.cmx_backend_recon_voxel_get_device, first, count, with_counts, out)

    def reconstruct_voxel_reset(self):
        """Clear the voxel volumes and their counters (after the knots have moved); the grids stay."""
        self._ck(self._L.cmx_backend_recon_voxel_reset(self._ctx))

    def reconstruct_voxel_end(self):
        self._ck(self._L.cmx_backend_recon_voxel_end(self._ctx))
        self._voxel_shape = None

    # --- time surfaces: the latest event per pixel and polarity of the same vote loop (cmx_backend_recon_surface_*)
    _surface_shape = None  # (n_surfaces, C, Hv, Wv) of the last reconstruct_surface_begin
    _surface_by_polarity = True

    def reconstruct_surface_begin(self, surfaces, Wv, Hv, by_polarity=True):
        """Attach time surfaces to the open reconstruction, every cell empty (trajectory.SURFACE_EMPTY).  surfaces: _lib.ReconView
        structures or tuples (quat_xyzw, fx, fy, cx, cy, t_lo_ns, t_hi_ns) -- trajectory.frame_views' or crop_view's output as it
        is; a range over all time is accepted.  by_polarity: two channels, ON then OFF; otherwise one, and polarity is never read."""
        n, arr = self._set_targets(surfaces)
        self._surface_shape = None
        self._ck(self._L.cmx_backend_recon_surface_begin(self._ctx, int(Wv), int(Hv), int(bool(by_polarity)), n, arr))
        self._surface_shape = (n, 2 if by_polarity else 1, int(Hv), int(Wv))
        self._surface_by_polarity = bool(by_polarity)

    def reconstruct_surface_add(self, x, y, t_ns, polarity=None):
        """reconstruct_add's vote loop over exactly these events: every sampled event is warped once into the world frame and its OWN
        timestamp is kept, where it is the latest, at the nearest pixel of every surface whose range holds it.  polarity (one value
        per event, nonzero / positive = ON) is needed for a by-polarity set and ignored by a merged one."""
        self._set_add(self._L.cmx_backend_recon_surface_add, x, y, t_ns, polarity, self._surface_by_polarity)

    def reconstruct_surface_add_aos(self, events, polarity_field="polarity"):
        """The same from a structured array of records with fields x, y, sec, nsec and a one-byte polarity field."""
        self._set_add_aos(self._L.cmx_backend_recon_surface_add_aos, events, polarity_field, self._surface_by_polarity)

    def reconstruct_surface_add_from(self, store, first, count):
        """The same over events_[first, first+count) of an EventStore (with polarity, EventStore.push(..., polarity=), for a
        by-polarity set)."""
        self._ck(self._L.cmx_backend_recon_surface_add_from(self._ctx, store._h, int(first), int(count)))

    def reconstruct_surface_get(self, first=0, count=None, with_counts=False, out=None):
        """(count, C, Hv, Wv) int64 timestamps of surfaces [first, first+count) in absolute nanoseconds, trajectory.SURFACE_EMPTY
        where no event landed [, int64 events that voted into each].  out: an object with data_ptr() -- a contiguous int64 torch
        tensor of that many elements on the context's device: the cells are written straight into it, nothing crosses the host,
        and out is returned in the array's place.  The call runs on the context's stream and returns when out is complete; work of
        the caller's that still writes the tensor on another stream must be finished."""
        return self._set_get(self._surface_shape or (0, 0, 0, 0), np.int64, self._L.cmx_backend_recon_surface_get,
                             self._L.cmx_backend_recon_surface_get_device, first, count, with_counts, out)

    def reconstruct_surface_decay(self, tau_ns, t_ref_ns=None, first=0, count=None, out=None):
        """(count, C, Hv, Wv) fp32: the surfaces read through exp(-(t_ref - T) / tau_ns) in one device pass -- 0 where no event
        landed, 1 where T >= t_ref.  t_ref_ns: one reference time per surface of the range (or one for all); None: every surface's
        own t_hi.  out: a contiguous float32 torch tensor on the context's device, as in reconstruct_surface_get."""
        count, shape = self._set_range(self._surface_shape or (0, 0, 0, 0), first, count)
        ref = None
        if t_ref_ns is not None:
            ref = np.ascontiguousarray(np.broadcast_to(np.asarray(t_ref_ns, np.int64), (shape[0],)))
        ref_p = ref.ctypes.data_as(c_i64p) if ref is not None else None
        if out is not None:
            self._ck(self._L.cmx_backend_recon_surface_decay_device(self._ctx, int(first), count, ref_p, float(tau_ns), out.data_ptr()))
            return out
        res = np.empty(shape, np.float32)
        self._ck(self._L.cmx_backend_recon_surface_decay(self._ctx, int(first), count, ref_p, float(tau_ns), res.ctypes.data_as(c_fp)))
        return res

    def reconstruct_surface_reset(self):
        """Set every cell back to empty and the counters to zero (after the knots have moved); the surfaces stay."""
        self._ck(self._L.cmx_backend_recon_surface_reset(self._ctx))

    def reconstruct_surface_end(self):
        self._ck(self._L.cmx_backend_recon_surface_end(self._ctx))
        self._surface_shape = None

    def reconstruct_get(self, with_counts=False):
        """The (Hp, Wp) fp32 plane [, events the sampling selected so far, events that voted so far]."""
        out = np.empty((self.Hp, self.Wp), np.float32)
        ns, ni = C.c_int64(), C.c_int64()
        self._ck(self._L.cmx_backend_recon_get(self._ctx, out.ctypes.data_as(c_fp), C.byref(ns) if with_counts else None,
                                               C.byref(ni) if with_counts else None))
        return (out, ns.value, ni.value) if with_counts else out

    def reconstruct_render(self, gamma=0.75, fov_quat=None):
        """publishEventImage's tone map on the reconstruction: (Hp, Wp) uint8, or (Hp, Wp, 3) BGR with the sensor outline."""
        q = _c(fov_quat, np.float64) if fov_quat is not None else None
        out = np.empty((self.Hp, self.Wp) if q is None else (self.Hp, self.Wp, 3), np.uint8)
        self._ck(self._L.cmx_backend_recon_render(self._ctx, float(gamma), _dp(q) if q is not None else None,
                                                  out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def reconstruct_end(self):
        self._ck(self._L.cmx_backend_recon_end(self._ctx))

    # --- whole-trajectory contrast and gradient on top of an open reconstruction (cmx_backend_recon_contrast .. _eval_from)
    def reconstruct_restart(self, knots_xyzw):
        """New knot values for the spline of reconstruct_begin (same K); plane, counters and gradient state start over."""
        k = _c(knots_xyzw, np.float64).reshape(-1, 4)
        if self._recon_K and k.shape[0] != self._recon_K:
            raise ValueError("restart takes the %d knots of begin, got %d" % (self._recon_K, k.shape[0]))
        self._ck(self._L.cmx_backend_recon_restart(self._ctx, _dp(k)))

    def reconstruct_contrast(self, sigma=1.0, measure=VARIANCE, want_grad=False):
        """Contrast of GaussianBlur(plane, sigma) over the plane as accumulated so far; want_grad opens a gradient pass
        (reconstruct_grad_add* over the same events in the same cuts, then reconstruct_grad_get)."""
        out = C.c_double()
        self._ck(self._L.cmx_backend_recon_contrast(self._ctx, float(sigma), int(measure), 1 if want_grad else 0, C.byref(out)))
        return out.value

    def reconstruct_grad_add(self, x, y, t_ns):
        x, y, t = _c(x, np.uint16), _c(y, np.uint16), _c(t_ns, np.int64)
        if not (len(x) == len(y) == len(t)):
            raise ValueError("x, y, t_ns must have equal length")
        self._ck(self._L.cmx_backend_recon_grad_add(self._ctx, len(x), x.ctypes.data_as(c_u16p), y.ctypes.data_as(c_u16p),
                                                    t.ctypes.data_as(c_i64p)))

    def reconstruct_grad_add_aos(self, events):
        ev = np.ascontiguousarray(events)
        lay = _lib.aos_layout_of(ev)
        self._ck(self._L.cmx_backend_recon_grad_add_aos(self._ctx, len(ev), ev.ctypes.data_as(C.c_void_p), C.byref(lay)))

    def reconstruct_grad_add_from(self, store, first, count):
        self._ck(self._L.cmx_backend_recon_grad_add_from(self._ctx, store._h, int(first), int(count)))

    def reconstruct_grad_get(self):
        """d(contrast) / d(left increment of every control pose): 3K doubles."""
        g = np.empty(3 * self._recon_K, np.float64)
        self._ck(self._L.cmx_backend_recon_grad_get(self._ctx, _dp(g)))
        return g

    def reconstruct_eval(self, store, first, count, knots=None, sigma=1.0, measure=VARIANCE, want_grad=True):
        """restart (when knots are given) + add_from + contrast [+ grad_add_from + grad_get] in one call: (contrast, grad | None)."""
        k = None
        if knots is not None:
            k = _c(knots, np.float64).reshape(-1, 4)
            if self._recon_K and k.shape[0] != self._recon_K:
                raise ValueError("eval takes the %d knots of begin, got %d" % (self._recon_K, k.shape[0]))
        out = C.c_double()
        g = np.empty(3 * self._recon_K, np.float64) if want_grad else None
        self._ck(self._L.cmx_backend_recon_eval_from(self._ctx, store._h, int(first), int(count), _dp(k) if k is not None else None,
                                                     float(sigma), int(measure), C.byref(out), _dp(g) if want_grad else None))
        return out.value, g

    # --- bound events (cmx_backend_recon_bind_from .. _bound_info): hand the events over once, evaluate them many times
    def reconstruct_bind(self, store, first, count):
        """Copy events_[first, first+count) of an EventStore -- those the sampling selects, and their batch times -- into the open
        reconstruction; the store may change or be closed afterwards.  A second call replaces the binding."""
        self._ck(self._L.cmx_backend_recon_bind_from(self._ctx, store._h, int(first), int(count)))

    def reconstruct_unbind(self):
        self._ck(self._L.cmx_backend_recon_unbind(self._ctx))

    def reconstruct_eval_bound(self, knots=None, sigma=1.0, measure=VARIANCE, want_grad=True):
        """reconstruct_eval over the bound events, always from a zeroed plane (knots None: the current ones), with the votes made
        through LDS over a tile sort kept from one evaluation to the next: (contrast, grad | None)."""
        k = None
        if knots is not None:
            k = _c(knots, np.float64).reshape(-1, 4)
            if self._recon_K and k.shape[0] != self._recon_K:
                raise ValueError("eval takes the %d knots of begin, got %d" % (self._recon_K, k.shape[0]))
        out = C.c_double()
        g = np.empty(3 * self._recon_K, np.float64) if want_grad else None
        self._ck(self._L.cmx_backend_recon_eval_bound(self._ctx, _dp(k) if k is not None else None, float(sigma), int(measure),
                                                      C.byref(out), _dp(g) if want_grad else None))
        return out.value, g

    def reconstruct_bound_info(self):
        """{'n_events', 'n_sampled', 'sorts' (tile sorts since the bind), 'fallback_frac' (share of the last evaluation's voting
        events that left their LDS window)}; all zero without a binding."""
        ne, ns, so, ff = C.c_int64(), C.c_int64(), C.c_int64(), C.c_double()
        self._ck(self._L.cmx_backend_recon_bound_info(self._ctx, C.byref(ne), C.byref(ns), C.byref(so), C.byref(ff)))
        return {"n_events": ne.value, "n_sampled": ns.value, "sorts": so.value, "fallback_frac": ff.value}

    def reconstruct_refine(self, store, first, count, order, knots, start_ns, dt_ns, num_fixed, sigma=1.0, measure=VARIANCE,
                           event_batch_size=100, event_sample_rate=1, bind=False, **solver_kw):
        """One bundle adjustment over the whole recording: FR-CG (the back end's constants unless given) over a left increment
        of every control pose but the first num_fixed, cost = -contrast of the panorama of events_[first, first+count).
        bind=True: the events are bound once and every trial point is a reconstruct_eval_bound.  Returns (knots, report)."""
        from . import solver
        k0 = np.array(_c(knots, np.float64).reshape(-1, 4), copy=True)
        K = k0.shape[0]
        nf = int(num_fixed)
        if not 0 <= nf < K:
            raise ValueError("num_fixed must be in [0, K)")
        kw = dict(solver.BACKEND)
        kw.update(solver_kw)

        def moved(x):
            k = k0.copy()
            self._ck(self._L.cmx_traj_incremental_update(K, _dp(k), nf, int(x.size), _dp(_c(x, np.float64))))
            return k

        def fdf(x, want_grad):
            if bind:
                c, g = self.reconstruct_eval_bound(moved(x), sigma, measure, want_grad)
            else:
                c, g = self.reconstruct_eval(store, first, count, moved(x), sigma, measure, want_grad)
            return -c, (-g[3 * nf:] if want_grad else None)

        self.reconstruct_begin(order, k0, start_ns, dt_ns, event_batch_size, event_sample_rate)
        try:
            if bind:
                self.reconstruct_bind(store, first, count)
            x, rep = solver.frcg_minimize(fdf, np.zeros(3 * (K - nf)), **kw)
        finally:
            self.reconstruct_end()
        return moved(x), rep

    # --- frozen head and the native solve (cmx_backend_recon_freeze_head / _frozen_info / _solve)
    def reconstruct_freeze_head(self, num_fixed):
        """Vote the batches whose pose reads only the first num_fixed knots ONCE, at the current knots, into a base plane; every
        later reconstruct_eval_bound starts from it and walks the other batches alone.  0 removes the frozen head."""
        self._ck(self._L.cmx_backend_recon_freeze_head(self._ctx, int(num_fixed)))

    def reconstruct_frozen_info(self):
        """{'num_fixed', 'frozen_batches', 'frozen_sampled'}; all zero without a frozen head."""
        nf, fb, fs = C.c_int(), C.c_int64(), C.c_int64()
        self._ck(self._L.cmx_backend_recon_frozen_info(self._ctx, C.byref(nf), C.byref(fb), C.byref(fs)))
        return {"num_fixed": nf.value, "frozen_batches": fb.value, "frozen_sampled": fs.value}

    def reconstruct_solve(self, knots, num_fixed, sigma=1.0, measure=VARIANCE, freeze_head=False, **solver_kw):
        """reconstruct_refine(bind=True)'s bundle adjustment over the events bound to the open reconstruction as ONE native call
        (FR-CG, the back end's constants unless given; freeze_head: the batches under the fixed knots are voted once).  The
        reconstruction is left at the refined knots' evaluation.  freeze_head="keep": under the frozen head as it stands
        (reconstruct_advance_head), with num_fixed the head's and its knots unchanged.  Returns (knots, report)."""
        from . import solver
        k = np.array(_c(knots, np.float64).reshape(-1, 4), copy=True)
        if self._recon_K and k.shape[0] != self._recon_K:
            raise ValueError("solve takes the %d knots of the reconstruction, got %d" % (self._recon_K, k.shape[0]))
        kw = dict(solver.BACKEND)
        kw.update(solver_kw)
        rep = _lib.SolveReport()
        if isinstance(freeze_head, str):
            if freeze_head != "keep":
                raise ValueError("freeze_head is False, True or 'keep'")
            mode = _lib.RECON_KEEP_HEAD
        else:
            mode = 1 if freeze_head else 0
        self._ck(self._L.cmx_backend_recon_solve(self._ctx, _dp(k), int(num_fixed), mode, float(sigma), int(measure),
                                                 float(kw["step_size"]), float(kw["tol"]), float(kw["epsabs_grad"]),
                                                 float(kw["tolfun"]), int(kw["max_iterations"]), C.byref(rep)))
        return k, {f: getattr(rep, f) for f, _ in rep._fields_}

    # --- a binding that grows (cmx_backend_recon_extend / _bind_append_from / _advance_head / _release_head / _online_info)
    def reconstruct_extend(self, knots_xyzw):
        """reconstruct_restart that may lengthen the spline (at least as many knots as now) and keeps a frozen head, whose
        knots must be unchanged; the binding stays."""
        k = _c(knots_xyzw, np.float64).reshape(-1, 4)
        self._ck(self._L.cmx_backend_recon_extend(self._ctx, k.shape[0], _dp(k)))
        self._recon_K = k.shape[0]

    def reconstruct_bind_append(self, store, first, count):
        """Append events_[first, first+count) of an EventStore to the binding: afterwards it is what reconstruct_bind over all
        ranges bound so far, concatenated, would hold.  Only this range is read from the store; a frozen head is kept."""
        self._ck(self._L.cmx_backend_recon_bind_append_from(self._ctx, store._h, int(first), int(count)))

    def reconstruct_advance_head(self, num_fixed):
        """Move the freeze line forward to num_fixed knots: the newly frozen batches vote once, at the current knots, on top
        of the base.  Without a frozen head: reconstruct_freeze_head."""
        self._ck(self._L.cmx_backend_recon_advance_head(self._ctx, int(num_fixed)))

    def reconstruct_release_head(self):
        """Free the resident memory of the frozen batches' events; evaluations are unchanged."""
        self._ck(self._L.cmx_backend_recon_release_head(self._ctx))

    def reconstruct_online_info(self):
        """{'released_batches', 'released_events', 'released_sampled', 'resident_sampled'}; all zero without a binding."""
        v = [C.c_int64() for _ in range(4)]
        self._ck(self._L.cmx_backend_recon_online_info(self._ctx, *[C.byref(a) for a in v]))
        return dict(zip(("released_batches", "released_events", "released_sampled", "resident_sampled"), (a.value for a in v)))

    def reconstruct_solve_counts(self):
        """(evaluations, host waits inside them) of the last reconstruct_solve (cmx_diag_recon_solve_counts)."""
        ev, hw = C.c_int64(), C.c_int64()
        self._ck(self._L.cmx_diag_recon_solve_counts(self._ctx, C.byref(ev), C.byref(hw)))
        return ev.value, hw.value

    def reconstruct(self, x, y, t_ns, order, knots_xyzw, start_ns, dt_ns, **kw):
        """begin + one add + get + end: the panorama of these events along this spline."""
        self.reconstruct_begin(order, knots_xyzw, start_ns, dt_ns, **kw)
        try:
            self.reconstruct_add(x, y, t_ns)
            return self.reconstruct_get()
        finally:
            self.reconstruct_end()

    # --- reference-named entry points
    def computeImageOfWarpedEvents(self, drotv, want_deriv=False):
        """iwe (blurred I = IL + alpha*IGp) [, list of blurred derivative planes] at the updated trajectory."""
        self.accumulate(drotv, want_deriv)
        iwe = self.get_plane(_lib.PLANE_IWE)
        if not want_deriv:
            return iwe
        return iwe, np.stack([self.get_plane(_lib.PLANE_DERIV0 + j) for j in range(self.num_params)])

    def contrast_fdf(self, v):
        c, g = self.eval(v, True)
        return -c, -g

    def contrast_f(self, v):
        return -self.eval(v, False)[0]

    def contrast_df(self, v):
        return -self.eval(v, True)[1]

    def setupProblemAndOptimize(self, drotv0=None):
        """FR-CG solve of the window (global_optim_contrast_gsl.cpp:15-145); the reference starts at 0.
        Returns (optimal incremental rotation vectors, report dict)."""
        x = np.zeros(self.num_params) if drotv0 is None else np.array(drotv0, dtype=np.float64, order="C", copy=True)
        rep = _lib.SolveReport()
        self._ck(self._L.cmx_backend_solve(self._ctx, int(self.num_params), _dp(x), C.byref(rep)))
        return x, {f: getattr(rep, f) for f, _ in rep._fields_}
