"""Device-resident generic nowcast loop, mirror of ``pysteps.nowcasts.utils.nowcast_main_loop``
(reference: pysteps/nowcasts/utils.py:265-533).

The reference advects every ensemble member once per time step through ``worker1`` / ``worker2``
(:441-462, :489-503): ``N_ens x T`` extrapolator calls, each moving 4+ full planes across PCIe when
the extrapolator is a GPU operator, each re-materialising the perturbed motion field
``V + generate_bps(...)`` in NumPy.  This loop keeps the same contract - signature, call order of
``func``, sub-time-step interpolation, callbacks, return value - and, when ``extrap_method``
resolves to the HIP extrapolator, advects ALL members with ONE launch of the member-batched
kernel (``EnsembleAdvector``): the trajectories ``D_j`` never leave HBM and the BPS velocity
perturbation (pysteps/noise/motion.py:146-180) is applied in-kernel from two scalars per member.
Anything it does not recognise (another extrapolator, perturbation generators that are not the
BPS closures of nowcasts/steps.py:931-933, exotic extrapolator options) takes the reference's own
member-by-member route through the extrapolator callable, so results never depend on the path.

``pysteps_amd.register.register(patch_main_loop=True)`` installs it in the pysteps modules that
imported the reference loop by name (steps, sprog, anvil, linda, ...).
"""

import time

import numpy as np

from .. import _lib
from .. import extrapolation as _hip_extrapolation
from .._reference import lookup, require
from ..device import DeviceArray
from ..extrapolation.ensemble import EnsembleAdvector
from ..extrapolation.semilagrangian import extrapolate as _hip_extrapolate

__all__ = ["nowcast_main_loop", "bps_perturbators", "compute_dilated_mask"]

MIN_HOST_MASK = 4096  # host masks below this many pixels stay with scipy.ndimage
# register(resident_update=...) / tests switch the resident STEPS member update (steps_resident.py) on and off
resident_update_enabled = True
# device time of the last resident run by phase (ms): {"upload", "update", "advect", "download"} -
# events on the library stream, read once at the end of the loop (tools/steps_quick.py, bench.py)
last_run_stats = {}


class _Timeline:
    """Events on the library stream between the phases of the loop; read once, at the end."""

    def __init__(self):
        import os  # noqa: PLC0415

        from ..device import Event  # noqa: PLC0415

        self._event = Event
        # PYSTEPS_HIP_LOOP_WALL=1: wait for the stream at every mark and use the host clock instead
        # (serialises the loop; for cross-checking the event figures)
        self.wall = os.environ.get("PYSTEPS_HIP_LOOP_WALL") == "1"
        self.marks = [("start", self._now())]

    def _now(self):
        if self.wall:
            _lib.check(_lib.lib().psh_sync(), "psh_sync")
            return time.perf_counter()
        return self._event().record()

    def mark(self, phase):
        self.marks.append((phase, self._now()))

    def totals(self):
        out = {}
        for (_, e0), (name, e1) in zip(self.marks[:-1], self.marks[1:]):
            out[name] = out.get(name, 0.0) + ((e1 - e0) * 1e3 if self.wall else e0.elapsed_ms(e1))
        return out


def compute_dilated_mask(input_mask, kr, r):
    """Buffer the input rain mask using the given kernel and add a grayscale rim (reference:
    pysteps/nowcasts/utils.py:69-101; parameters and return value as documented there).

    ``psh_dilated_mask_dev`` (csrc/mask.hip): one dilation by ``kr`` and a truncated L1 distance
    transform instead of ``1 + r`` calls of ``scipy.ndimage.binary_dilation``; bit-identical output.
    A ``DeviceArray`` mask (uint8, non-zero = set) gives a ``DeviceArray``.  Masks that are not
    two-dimensional, more than 254 rim iterations, structuring elements with more than 1024 set
    elements and small host masks go to the reference's function."""
    import ctypes  # noqa: PLC0415

    from .. import _lib  # noqa: PLC0415
    from ..device import DeviceArray  # noqa: PLC0415

    resident = isinstance(input_mask, DeviceArray)
    struct = np.ascontiguousarray(np.asarray(kr) != 0, dtype=np.uint8)
    shape = tuple(input_mask.shape) if resident else np.shape(input_mask)
    eligible = (
        len(shape) == 2 and struct.ndim == 2 and struct.size > 0 and isinstance(r, (int, np.integer))
        and 0 <= r <= 254 and int(struct.sum()) <= 1024 and shape[0] > 0 and shape[1] > 0
    )
    if resident:
        if not eligible or input_mask.dtype != np.uint8:
            raise NotImplementedError("device-resident masks: two-dimensional uint8, r <= 254, <= 1024 structure elements")
        d_mask = input_mask
    else:
        if not eligible or shape[0] * shape[1] < MIN_HOST_MASK:
            return require("nowcasts.utils", "compute_dilated_mask", compute_dilated_mask)(input_mask, kr, r)
        # utils.py:87: the mask is cast to uint8 first (a value of 0.5 becomes 0, 256 wraps to 0)
        d_mask = DeviceArray.from_host(np.ndarray.astype(np.asarray(input_mask), "uint8"), sync=False)
    out = DeviceArray(shape, np.float64)
    _lib.check(
        _lib.lib().psh_dilated_mask_dev(d_mask.ptr, int(shape[0]), int(shape[1]),
                                        struct.ctypes.data_as(ctypes.c_void_p), int(struct.shape[0]),
                                        int(struct.shape[1]), int(r), out.ptr),
        "psh_dilated_mask_dev",
    )
    return out if resident else out.to_host()

_BPS_KEYS = ("eps_par", "eps_perp", "p_par", "p_perp", "vsf", "V_par", "V_perp")


def _time_bins(timesteps):
    """[(integer step t, [lead times in [t, t+1)], announce)] - the iteration plan of the
    reference (create_timestep_range / binned_timesteps, utils.py:34-66,247-262)."""
    if isinstance(timesteps, int):
        return [(t, [t], t > 0) for t in range(timesteps + 1)]
    ts = [0] + list(timesteps)
    if sorted(ts) != ts:
        raise ValueError("timesteps is not in ascending order")
    if min(ts) < 0:
        raise ValueError("negative time steps are not allowed")
    last = int(np.ceil(ts[-1]))
    bins = [[] for _ in range(last + 1)]
    for v in ts:
        # np.digitize(v, arange(last + 1), right=False) - 1
        bins[min(int(np.floor(v)), last)].append(v)
    return [(t, sub, bool(sub)) for t, sub in enumerate(bins)]


def bps_perturbators(velocity_pert_gen, velocity):
    """The scalar BPS parameters behind a list of perturbation generators, or None.

    nowcasts/steps.py:931-933 wraps each perturbator dict of ``initialize_bps`` in
    ``lambda t, vp=vp: generate_vel_noise(vp, t * timestep)``.  The dict is the lambda's default
    argument; the time scale is recovered by calling the generator once on a 1x1 stand-in
    perturbator, and the claim "perturbation = par(t) V/|V| + perp(t) (V/|V|)_perp of THIS motion
    field" is verified against one full evaluation before it is trusted."""
    out = []
    for fn in velocity_pert_gen:
        vp = (getattr(fn, "__defaults__", None) or (None,))[-1]
        if not isinstance(vp, dict) or any(k not in vp for k in _BPS_KEYS):
            return None
        probe = dict(vp)
        one = np.ones((2, 1, 1))
        probe.update(V_par=one, V_perp=0 * one, eps_par=1.0, eps_perp=0.0, p_par=(1.0, 1.0, 0.0),
                     p_perp=(0.0, 1.0, 0.0), vsf=1.0)
        try:
            scale = float(np.ravel(fn(1.0, vp=probe))[0])  # = 1.0 * timestep
        except Exception:
            return None
        if not np.isfinite(scale) or scale <= 0:
            return None
        out.append(dict(eps_par=float(vp["eps_par"]), eps_perp=float(vp["eps_perp"]), p_par=tuple(vp["p_par"]),
                        p_perp=tuple(vp["p_perp"]), vsf=float(vp["vsf"]), time_scale=scale))
    if not out:
        return None
    # EVERY generator against its closed form on this motion field, on a jittered lattice of ~512 x 512 samples:
    # one sample per cell of `step` x `step` pixels at a position inside the cell that is a FIXED pseudo-random
    # function of the cell (seeded generator: the same inputs get the same verdict on every call and in every
    # process - round-4 advisor), so that neither a shifted / filtered motion field (differs everywhere) nor a
    # difference confined to the rows or columns of one residue class goes unseen.  One evaluation on the full
    # 4096^2 grid would cost 0.4 s of a 1.2 s main loop.  The closed form follows noise/motion.py:129-133 in the
    # velocity's own dtype: a float32 motion field is normalised in float32 there
    vel = np.asarray(velocity)
    if vel.ndim != 3 or vel.shape[0] != 2:
        return None
    step = max(1, min(vel.shape[1:]) // 512)
    sub = _jittered_lattice(vel.shape[1], vel.shape[2], step)
    vel = np.ascontiguousarray(vel[sub])
    if vel.dtype.kind != "f":
        vel = vel.astype(np.float64)
    rtol = 1e-9 if vel.dtype.itemsize >= 8 else 1e-6
    norm = np.linalg.norm(vel, axis=0)
    unit = np.where(norm > 1e-12, vel / np.where(norm > 1e-12, norm, 1.0), 0.0).astype(np.float64)
    perp = np.stack([-unit[1], unit[0]])
    t = 1.5
    for fn, p in zip(velocity_pert_gen, out):
        vp = fn.__defaults__[-1]
        tm = t * p["time_scale"]
        g_par = p["p_par"][0] * pow(tm, p["p_par"][1]) + p["p_par"][2]
        g_perp = p["p_perp"][0] * pow(tm, p["p_perp"][1]) + p["p_perp"][2]
        closed = (g_par * p["eps_par"] * unit + g_perp * p["eps_perp"] * perp) / p["vsf"]
        try:
            if np.shape(vp["V_par"]) != np.shape(velocity) or np.shape(vp["V_perp"]) != np.shape(velocity):
                return None
            thin = dict(vp, V_par=np.asarray(vp["V_par"])[sub], V_perp=np.asarray(vp["V_perp"])[sub])
            if not np.allclose(fn(t, vp=thin), closed, rtol=rtol, atol=1e-12):
                return None
        except Exception:
            return None
    return out


def _jittered_lattice(m, n, step):
    """Index (slice(None), rows, cols) of one pixel per ``step`` x ``step`` cell of an (m, n) grid; the position
    inside a cell comes from a generator with a fixed seed (deterministic, see bps_perturbators)."""
    if step <= 1:
        return (slice(None), slice(None), slice(None))
    cy, cx = -(-m // step), -(-n // step)
    rng = np.random.default_rng(0x5EED)
    iy = np.minimum(np.arange(cy)[:, None] * step + rng.integers(0, step, size=(cy, cx)), m - 1)
    ix = np.minimum(np.arange(cx)[None, :] * step + rng.integers(0, step, size=(cy, cx)), n - 1)
    return (slice(None), iy, ix)


def _batched_options(extrap_kwargs):
    """Options of the extrapolator the member-batched kernel implements -> dict, else None."""
    kw = dict(extrap_kwargs)
    for k in ("xy_coords", "return_displacement", "displacement_prev", "allow_nonfinite_values", "verbose"):
        kw.pop(k, None)
    opts = dict(n_iter=int(kw.pop("n_iter", 1)), interp_order=kw.pop("interp_order", 1),
                outval=kw.pop("outval", np.nan))
    if kw.pop("map_coordinates_mode", "constant") != "constant" or kw.pop("vel_timestep", 1) != 1 or kw:
        return None
    if opts["interp_order"] not in (0, 1) or isinstance(opts["outval"], str) or opts["n_iter"] < 0:
        return None
    return opts


class _MemberLoop:
    """The reference's route: one extrapolator call per member (utils.py:441-462, 489-503)."""

    def __init__(self, extrapolator, velocity, shape, extrap_kwargs, velocity_pert_gen):
        self.extrapolator, self.velocity, self.gen = extrapolator, velocity, velocity_pert_gen
        m, n = shape
        xg, yg = np.meshgrid(np.arange(n), np.arange(m))
        self.kw = dict(extrap_kwargs, xy_coords=np.stack([xg, yg]), return_displacement=True)
        self.disp = None

    def advect(self, fields, n_members, dt, t_total):
        if self.disp is None:
            self.disp = [None] * n_members
        if isinstance(fields, DeviceArray):  # resident member update, foreign extrapolator: through the host
            fields = fields.to_host()
        res = []
        for j in range(n_members):
            kw = dict(self.kw, displacement_prev=self.disp[j])
            v = self.velocity if self.gen is None else self.velocity + self.gen[j](t_total)
            if fields is None:
                _, self.disp[j] = self.extrapolator(None, v, [dt], **kw)
            else:
                kw["allow_nonfinite_values"] = bool(np.any(~np.isfinite(fields[j])))
                out, self.disp[j] = self.extrapolator(fields[j], v, [dt], **kw)
                res.append(out[0])
        return res if fields is not None else None


class _BatchedLoop:
    """All members in one launch, trajectories resident in HBM."""

    def __init__(self, velocity, perturbators, opts):
        self.velocity, self.perts, self.opts = velocity, perturbators, opts
        self.adv = None
        self.timeline = None
        self.moved = None  # float32 DeviceArray of the members advected last from resident fields

    def advect(self, fields, n_members, dt, t_total, sink=None, on_device=False):
        """``on_device`` (resident fields only): no download - the float32 stack of the advected members is returned as
        the advector left it in HBM.  It is valid until the next call (the advector may reuse it)."""
        if self.adv is None:
            self.adv = EnsembleAdvector(self.velocity, n_members, self.perts, **self.opts)
        lead = None if self.perts is None else t_total * self.perts[0]["time_scale"]  # minutes
        if fields is None:
            self.adv.step(None, dt, lead)
            return None
        if isinstance(fields, DeviceArray):
            # resident member update: float64 fields in HBM -> float32 for the kernel -> ONE transfer of
            # the advected members per output time step, widened to the reference's float64 on the device
            f32 = DeviceArray(fields.shape, np.float32)
            _lib.check(_lib.lib().psh_convert_dev(fields.ptr, f32.ptr, fields.size, 0), "psh_convert_dev")
            moved = self.adv.step(f32, dt, lead)
            if self.timeline is not None:
                self.timeline.mark("advect")
            self.moved = moved
            if on_device and sink is None:
                return moved
            if sink is not None:
                # straight into the caller's (n_members, n_timesteps, m, n) result block: widened on the
                # device, one queued copy per member, nobody waits here
                wide = DeviceArray(moved.shape, np.float64)
                lib = _lib.lib()
                _lib.check(lib.psh_convert_dev(moved.ptr, wide.ptr, moved.size, 1), "psh_convert_dev")
                plane_bytes = wide.nbytes // n_members
                for j in range(n_members):
                    _lib.check(lib.psh_memcpy_d2h_async(sink[j].ctypes.data, wide.ptr + j * plane_bytes, plane_bytes), "d2h")
                if self.timeline is not None:
                    self.timeline.mark("download")
                return list(sink)
            got = moved.to_host(dtype=fields.dtype)
            if self.timeline is not None:
                self.timeline.mark("download")
        else:
            got = self.adv.step(np.asarray(fields), dt, lead, out_dtype=np.asarray(fields).dtype)
        return [got[j] for j in range(n_members)]


def nowcast_main_loop(precip, velocity, state, timesteps, extrap_method, func, extrap_kwargs=None,
                      velocity_pert_gen=None, params=None, ensemble=False, num_ensemble_members=1,
                      callback=None, return_output=True, num_workers=1, measure_time=False):
    """Same parameters, call order and return value as the reference (utils.py:265-345): a list /
    array of forecast fields ``(n_timesteps, m, n)`` or ``(n_members, n_timesteps, m, n)``, with the
    loop time when ``measure_time`` is set.  ``num_workers`` is accepted; the members are advanced
    together on the GPU instead of by worker threads.

    A ``callback`` with a truthy ``accepts_device`` attribute (``postprocessing.ensemblestats.EnsembleProducts``) is
    called with the float32 ``DeviceArray`` ``(n_members, m, n)`` of the advected members while the loop runs the
    resident update with the member-batched advection - valid during the call only, the advector may reuse it - and
    with ``return_output=False`` no member is then widened or copied to the host (``last_run_stats`` has a ``callback``
    and no ``download`` phase).  In every other case such a callback gets the host stack like any other."""
    started = time.time()  # like the reference (utils.py:347): set-up of the loop is part of its time
    plan = _time_bins(timesteps)
    extrap_kwargs = {} if extrap_kwargs is None else dict(extrap_kwargs)
    # the ANVIL update of nowcasts/anvil.py with its cascade state in HBM: a single field per step, advected by the
    # HIP extrapolator whatever pysteps' own table maps the name to
    anvil = None
    if not ensemble:
        from .anvil import try_create as anvil_resident  # noqa: PLC0415

        anvil = anvil_resident(func, state)
    get_extrapolator = None if anvil is not None else lookup("extrapolation", "get_method", None)
    extrapolator = (get_extrapolator or _hip_extrapolation.get_method)(extrap_method)

    n_members = num_ensemble_members if ensemble else 1
    engine = None
    if extrapolator is _hip_extrapolate:
        opts = _batched_options(extrap_kwargs)
        if opts is not None and not np.all(np.isfinite(velocity)):
            # the reference's extrapolator decides what a non-finite motion field means (ValueError unless
            # allow_nonfinite_values, semilagrangian.py:106-137): such fields go member by member through it
            opts = None
        perts = None
        if velocity_pert_gen is not None and opts is not None:
            perts = bps_perturbators(velocity_pert_gen, velocity)
            if perts is None:
                opts = None
        if opts is not None:
            engine = _BatchedLoop(np.asarray(velocity), perts, opts)
    if engine is None:
        engine = _MemberLoop(extrapolator, velocity, precip.shape, extrap_kwargs, velocity_pert_gen)

    # the STEPS member update with all of its state in HBM (steps_resident.py), when `func` is the
    # reference's StepsNowcaster.__update_state and its options are the ones the chain implements
    # (only together with the HIP extrapolator: a caller who chose another one keeps the reference's update)
    resident = timeline = None
    if ensemble and resident_update_enabled and extrapolator is _hip_extrapolate:
        from .steps_resident import recognises, try_create  # noqa: PLC0415

        if recognises(func):
            timeline = _Timeline()
            resident = try_create(func, state, params, precip.shape, len(plan))
            if resident is None:
                timeline = None
            else:
                timeline.mark("upload")
                if isinstance(engine, _BatchedLoop):
                    engine.timeline = timeline

    if anvil is not None:
        resident, timeline = anvil, _Timeline()
        timeline.mark("upload")

    prev = np.stack([precip] * n_members) if ensemble else precip[np.newaxis, :]
    outputs = [[] for _ in range(prev.shape[0])] if return_output else None
    # resident update + member-batched advection: the advected members of every output time step are
    # copied straight into ONE (n_members, n_timesteps, m, n) block (pinned if the pool has room) by
    # queued copies; the loop waits for them once at the end (and before every callback)
    block = None
    if resident is not None and isinstance(engine, _BatchedLoop) and return_output:
        from .. import _pinned  # noqa: PLC0415

        n_out = sum(1 for _, sub, _ in plan for ts in sub if ts > 0)
        if n_out:
            block = _pinned.empty((n_members, n_out) + tuple(precip.shape), np.float64)
            if timeline is not None:
                timeline.mark("result_block")
    # a callback that takes the members where they lie (``accepts_device``, e.g. postprocessing.ensemblestats.EnsembleProducts)
    # gets the float32 DeviceArray (n_members, m, n) the advector returned instead of np.stack(advected); it is valid
    # during the call only, the advector may reuse it.  With return_output=False no member is widened or downloaded
    device_callback = (callback is not None and bool(getattr(callback, "accepts_device", False))
                       and resident is not None and isinstance(engine, _BatchedLoop))
    out_index = 0
    t_prev = t_total = 0.0
    try:
        for t, subtimesteps, announce in plan:
            if announce:
                print(f"Computing nowcast for time step {t}... ", end="", flush=True)
                step_started = time.time()
            if resident is not None:
                new = resident.update()
                timeline.mark("update")
            else:
                new, state = func(state, params)
                if not ensemble:
                    new = new[np.newaxis, :]
            for t_sub in subtimesteps:
                if not t_sub > 0:
                    continue
                w = t_sub - int(t_sub)  # linear interpolation between the integer-step fields (:419-427)
                if resident is not None and w > 0.0:
                    if not isinstance(prev, DeviceArray):
                        prev = DeviceArray.from_host(np.ascontiguousarray(prev, dtype=np.float64))
                    fields = DeviceArray(new.shape, np.float64)
                    _lib.check(_lib.lib().psh_lerp_dev(prev.ptr, new.ptr, float(w), fields.ptr, new.size), "psh_lerp_dev")
                else:
                    fields = (1.0 - w) * prev + w * new if w > 0.0 else prev
                dt = t_sub - t_prev
                t_total += dt
                if block is not None:
                    advected = engine.advect(fields, fields.shape[0], dt, t_total, sink=block[:, out_index])
                    out_index += 1
                    if callback is not None and not device_callback:
                        _lib.check(_lib.lib().psh_sync(), "psh_sync")
                elif device_callback and isinstance(fields, DeviceArray) and not return_output:
                    advected = engine.advect(fields, fields.shape[0], dt, t_total, on_device=True)
                else:
                    advected = engine.advect(fields, fields.shape[0], dt, t_total)
                    if return_output:
                        for j, a in enumerate(advected):
                            outputs[j].append(a)
                if device_callback and isinstance(fields, DeviceArray):
                    callback(engine.moved)
                    timeline.mark("callback")
                elif callback is not None:
                    callback(np.stack(advected))
                t_prev = t_sub
            if not subtimesteps:  # no lead time in this bin: displacement only, up to the next integer step
                dt = t + 1 - t_prev
                t_total += dt
                engine.advect(None, new.shape[0], dt, t_total)
                t_prev = t + 1
            prev = new
            if announce:
                print(f"{time.time() - step_started:.2f} seconds." if measure_time else "done.")
    except BaseException:
        # a callback, a HIP error or a failed matching ended the loop: the generators' side stream is joined and
        # the host RandomStates get their streams back before the device buffers are released
        if resident is not None:
            resident.abort()
            resident = None
        raise

    if resident is not None:
        resident.finish()
        last_run_stats.clear()
        last_run_stats.update(timeline.totals())
        last_run_stats["members"], last_run_stats["updates"] = n_members, len(plan)
    result = None
    if block is not None:
        _lib.check(_lib.lib().psh_sync(), "psh_sync")
        result = block if ensemble else block[0]
    elif return_output:
        result = np.stack([np.stack(o) for o in outputs])
        if not ensemble:
            result = result[0, :]
    return (result, time.time() - started) if measure_time else result
