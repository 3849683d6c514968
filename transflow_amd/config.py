"""Parameter objects of the hot path, mirroring the reference's own
(same names, defaults and parsing), so a config built for transflow drives this
backend unchanged.

  LayerConfig   <- transflow/config.py:57-104   (fields the compositor reads)
  FlowConfig    <- CvFlowConfig, transflow/flow/sources/cv.py:271-363 (the fb_* fields)
  HornSchunckConfig <- the same, method "horn-schunck" (the hs_* fields)
  LucasKanadeConfig <- the same, method "lukas-kanade" (the lk_* fields; opt-in: lucas_kanade=True)
  LiteFlowNetConfig <- the same, method "liteflownet" (no fields; opt-in: liteflownet=<weights path or dict>;
                       hip_lfn_precision chooses how its convolutions multiply)

`hip_resident` (every method; for Farnebäck it matters with fb_flags & 4 only) keeps a method's flows, and the previous
output a chaining call starts from, on the device; with it the other three methods take hip_device_flows and hip_batch.

The four are MethodConfig subclasses; METHODS is the one table of the methods served and of what opts each in, which
the flow_config_from_* readers (and through them HipFlowSource.from_args and the drop-in) ask.
"""
from __future__ import annotations

import json
import os

_TRUE_WORDS = ("1", "on", "o", "oui", "yes", "y")  # config.py:49-54


def parse_bool_arg(arg, default: bool) -> bool:
    if arg is None:
        return default
    if isinstance(arg, str):
        return arg.lower().strip() in _TRUE_WORDS
    return arg


class LayerConfig:
    """Same constructor and attributes as the reference's LayerConfig."""

    _BOOLS = (
        ("transparent_pixels_can_move", False), ("pixels_can_move_to_empty_spot", True),
        ("pixels_can_move_to_filled_spot", True), ("moving_pixels_leave_empty_spot", False),
        ("reset_source", False), ("introduce_pixels_on_empty_spots", True),
        ("introduce_pixels_on_filled_spots", True), ("introduce_moving_pixels", True),
        ("introduce_unmoving_pixels", True), ("introduce_once", False),
        ("introduce_on_all_filled_spots", False), ("introduce_on_all_empty_spots", False),
    )

    def __init__(self, index: int, classname: str | None = None, mask_alpha: str | None = None,
                 mask_src: str | None = None, mask_dst: str | None = None,
                 transparent_pixels_can_move=None, pixels_can_move_to_empty_spot=None,
                 pixels_can_move_to_filled_spot=None, moving_pixels_leave_empty_spot=None,
                 reset_mode: str | None = None, reset_mask: str | None = None,
                 reset_random_factor: float | None = None, reset_constant_step: float | None = None,
                 reset_linear_factor: float | None = None, reset_source=None,
                 introduce_pixels_on_empty_spots=None, introduce_pixels_on_filled_spots=None,
                 introduce_moving_pixels=None, introduce_unmoving_pixels=None, introduce_once=None,
                 introduce_on_all_filled_spots=None, introduce_on_all_empty_spots=None):
        given = locals()
        self.index = index
        self.classname = "moveref" if classname is None else classname
        self.mask_alpha, self.mask_src, self.mask_dst = mask_alpha, mask_src, mask_dst
        for name, default in self._BOOLS:
            setattr(self, name, parse_bool_arg(given[name], default))
        self.reset_mode = "off" if reset_mode is None else reset_mode
        self.reset_mask = reset_mask
        self.reset_random_factor = 1 if reset_random_factor is None else reset_random_factor
        self.reset_constant_step = 1 if reset_constant_step is None else reset_constant_step
        self.reset_linear_factor = 0.1 if reset_linear_factor is None else reset_linear_factor

    _KEYS = ("index", "classname", "mask_src", "mask_dst", "mask_alpha", "transparent_pixels_can_move",
             "pixels_can_move_to_empty_spot", "pixels_can_move_to_filled_spot", "moving_pixels_leave_empty_spot",
             "reset_mode", "reset_mask", "reset_random_factor", "reset_constant_step", "reset_linear_factor",
             "reset_source", "introduce_pixels_on_empty_spots", "introduce_pixels_on_filled_spots",
             "introduce_moving_pixels", "introduce_unmoving_pixels", "introduce_once",
             "introduce_on_all_filled_spots", "introduce_on_all_empty_spots")

    def todict(self) -> dict:
        return {k: getattr(self, k) for k in self._KEYS}

    @classmethod
    def fromdict(cls, d: dict):
        kw = {k: d[k] for k in cls._KEYS if k in d and k != "index"}
        kw.setdefault("classname", "reference")  # config.py:110
        return cls(d["index"], **kw)

    @classmethod
    def from_reference(cls, cfg):
        """Accepts a transflow.config.LayerConfig (or anything with the same attributes)."""
        if isinstance(cfg, cls):
            return cfg
        return cls(cfg.index, **{k: getattr(cfg, k) for k in cls._KEYS if k != "index" and hasattr(cfg, k)})


def _exact_sums(v):
    return bool(parse_bool_arg(v, False))


def _lfn_precision(v):
    if v is None:
        return "f32"
    if not isinstance(v, str) or v not in ("f32", "bf16", "bf16x3"):
        raise ValueError(f"hip_lfn_precision {v!r} is not 'f32', 'bf16' or 'bf16x3'")
    return v


def _device_flows(v):
    return "ipc" if isinstance(v, str) and v.lower() == "ipc" else parse_bool_arg(v, False)


# This backend's own keys in a CvFlowConfig JSON, each with what makes its attribute of the value given (None: the key
# is not there); to_dict() writes them in this order, and only where they differ from their default.  The reference
# ignores keys it does not know only if they are not there: leave them out of files the reference itself must read.
_HIP_KEYS = {
    # "hip_exact_sums": true asks for the box window summed in OpenCV's own order (library option fb_exact_sums: flows
    # bit-identical to the CPU path's, about 1.5 times the Farnebäck time for a single 4K pair).
    "hip_exact_sums": _exact_sums,
    # "hip_prefetch": n > 0 lets the flow source run up to n flows ahead of its consumer in a worker thread with a
    # library stream of its own (what the reference gets from running the source in a child process behind a
    # queue, pipeline.py:56-64, for a source used in-process).  Its position attributes then run ahead by as much.
    "hip_prefetch": lambda v: int(v or 0),
    # "hip_device_flows": true -- the source yields DeviceFlow objects (transflow_amd/deviceflow.py): flows that stay in
    # HBM until something reads them on the host, and that HipCompositor.update takes by device address (no 66 MB per
    # 4K frame down the link and up again across pipeline.py:562-567).  "ipc": the same, and through a multiprocessing
    # queue (pipeline.py:85-86) such a flow travels as a 64-byte HIP IPC handle instead of the pickled array.
    "hip_device_flows": _device_flows,
    # "hip_batch": n > 1 -- where nothing can look at a raw flow in between (no lock expressions, no convolution kernel,
    # no initial flow), the source reads n frames ahead and computes their n pairs in ONE Farneback call: a single 4K
    # pair leaves most of the chip idle at the coarse levels, a batch of four costs 0.6 of four single calls.  Flows
    # still come out one at a time, in order, each post-processed with its own t.
    "hip_batch": lambda v: max(1, int(v or 1)),
    # "hip_lfn_precision": "bf16" or "bf16x3" -- LiteFlowNet's convolutions multiply bfloat16 operands on the bf16 matrix
    # cores ("bf16": both operands rounded to bfloat16; "bf16x3": each split into a bfloat16 pair, three products) and
    # sum in float32; "f32" (the default) is float32 throughout.  Only the liteflownet method takes it.
    "hip_lfn_precision": _lfn_precision,
    # "hip_resident": true -- Horn-Schunck, Lucas-Kanade and LiteFlowNet flows (and Farnebäck's when fb_flags has
    # cv2.OPTFLOW_USE_INITIAL_FLOW) stay on the device from the kernel that makes them through the filters, the mask and
    # the direction handling, and the previous output a call starts from is kept there too: one flow comes down per
    # frame, or none with "hip_device_flows".  Off (the default) every source takes the route it took before the key
    # existed.  Without it the three methods refuse "hip_device_flows" and "hip_batch": there is no resident flow.
    "hip_resident": lambda v: bool(parse_bool_arg(v, False)),
}


class MethodConfig:
    """One flow method's part of CvFlowConfig (cv.py:271-363): the method's own fields with their defaults as
    attributes, the `hip_*` keys it accepts, and every other key carried in `.extra` so that a CvFlowConfig JSON
    loads and is written back whole.  A subclass states the method's name, its fields and its `hip_*` keys."""

    METHOD = None
    DEFAULTS: dict = {}
    HIP_KEYS: tuple = ()        # the keys of _HIP_KEYS the method accepts; another `hip_*` key is a ValueError
    # ... and those of the resident route, "hip_resident" first: the others are accepted only where it is true
    RESIDENT_KEYS: tuple = ("hip_resident", "hip_device_flows", "hip_batch")
    # the attributes of the keys a method does not accept: what they mean when they are not given
    hip_exact_sums, hip_prefetch, hip_device_flows, hip_batch = False, 0, False, 1
    hip_lfn_precision = "f32"
    hip_resident = False

    def __init__(self, method: str, **kwargs):
        if method != self.METHOD:
            raise ValueError(self._wrong_method(method))
        self.method = method
        for k, v in self.DEFAULTS.items():
            setattr(self, k, kwargs.pop(k, v))
        accepted = self._accepted_keys(kwargs)
        for k in kwargs:
            if k.startswith("hip_") and k not in accepted:
                self._refuse_hip_key(k)
        for k in accepted:
            setattr(self, k, _HIP_KEYS[k](kwargs.pop(k, None)))
        self.extra = dict(kwargs)  # the other methods' fields, show_window ...: not used by this backend

    def _wrong_method(self, method) -> str:
        return f"{type(self).__name__} is the {self.METHOD!r} method, got {method!r}"

    def _accepted_keys(self, given: dict) -> tuple:
        """HIP_KEYS, and of RESIDENT_KEYS the switch alone unless it is given and true."""
        switch = self.RESIDENT_KEYS[:1]
        on = bool(switch) and _HIP_KEYS[switch[0]](given.get(switch[0]))
        return self.HIP_KEYS + (self.RESIDENT_KEYS if on else switch)

    def _refuse_hip_key(self, key):
        if key in self.RESIDENT_KEYS:
            raise ValueError(f"{key!r} is not available with the {self.METHOD} method without 'hip_resident': true "
                             "(its flows come down raw and are post-processed from the host array)")
        keys = self.HIP_KEYS + self.RESIDENT_KEYS
        only = f" (only {', '.join(map(repr, keys))} {'are' if len(keys) > 1 else 'is'}, the last two with 'hip_resident')"
        raise ValueError(f"{key!r} is not available with the {self.METHOD} method{only}")

    def to_dict(self) -> dict:
        d = {"method": self.method}
        d.update({k: getattr(self, k) for k in self.DEFAULTS})
        d.update(self.extra)
        for k in _HIP_KEYS:
            if k in self.HIP_KEYS + self.RESIDENT_KEYS and getattr(self, k) != _HIP_KEYS[k](None):
                d[k] = getattr(self, k)
        return d

    def to_file(self, path: str):
        with open(path, "w", encoding="utf8") as f:
            json.dump(self.to_dict(), f, indent=4)

    @classmethod
    def from_reference(cls, cfg, **given):
        """A reference CvFlowConfig (or anything with its attributes, or None) -> this method's fields of it."""
        if isinstance(cfg, cls):
            return cfg
        return cls(**{k: getattr(cfg, k) for k in cls.DEFAULTS if hasattr(cfg, k)}, **given)


def _from_file(cls, path: str):
    with open(path, "r", encoding="utf8") as f:
        return cls(**json.load(f))


class FlowConfig(MethodConfig):
    """The Farnebäck fields of CvFlowConfig (cv.py:273-281) and their defaults; other
    methods' fields (hs_*, lk_*) are accepted and carried so a CvFlowConfig JSON loads."""

    METHOD = "farneback"
    DEFAULTS = FB_DEFAULTS = dict(fb_pyr_scale=0.5, fb_levels=3, fb_winsize=15, fb_iterations=3, fb_poly_n=5,
                                  fb_poly_sigma=1.2, fb_flags=0)
    HIP_KEYS = ("hip_exact_sums", "hip_prefetch", "hip_device_flows", "hip_batch")
    RESIDENT_KEYS = ("hip_resident",)       # matters with fb_flags & 4 only: without that flag Farnebäck is resident anyway
    from_file = classmethod(_from_file)

    def __init__(self, method: str = "farneback", **kwargs):
        super().__init__(method, **kwargs)

    def _wrong_method(self, method) -> str:
        return f"transflow_amd implements the 'farneback' method only, got {method!r}"

    def _refuse_hip_key(self, key):
        pass                       # (a `hip_*` key this backend does not know is carried in `.extra` like any other)

    def fb_kwargs(self) -> dict:
        return dict(pyr_scale=self.fb_pyr_scale, levels=self.fb_levels, winsize=self.fb_winsize,
                    iterations=self.fb_iterations, poly_n=self.fb_poly_n, poly_sigma=self.fb_poly_sigma,
                    flags=self.fb_flags)


class HornSchunckConfig(MethodConfig):
    """The Horn-Schunck fields of CvFlowConfig (cv.py:282-285) and their defaults; `hs_delta` may be None (JSON null:
    every call runs hs_iterations iterations).  fb_*, lk_* and other keys are carried in `.extra`."""

    METHOD = "horn-schunck"
    DEFAULTS = HS_DEFAULTS = dict(hs_alpha=1, hs_iterations=3, hs_decay=0, hs_delta=1)
    HIP_KEYS = ("hip_prefetch",)
    from_file = classmethod(_from_file)

    def __init__(self, method: str = "horn-schunck", **kwargs):
        super().__init__(method, **kwargs)

    def hs_kwargs(self) -> dict:
        """The keyword arguments of calc_optical_flow_horn_schunck (cv.py:495-498)."""
        return dict(alpha=self.hs_alpha, max_iters=self.hs_iterations, decay=self.hs_decay, delta=self.hs_delta)


class LucasKanadeConfig(MethodConfig):
    """The Lucas-Kanade fields of CvFlowConfig and their defaults (lk_window_size 15, lk_max_level 2, lk_step 1).
    fb_*, hs_* and other keys are carried in `.extra`."""

    METHOD = "lukas-kanade"
    DEFAULTS = LK_DEFAULTS = dict(lk_window_size=15, lk_max_level=2, lk_step=1)
    HIP_KEYS = ("hip_prefetch",)
    from_file = classmethod(_from_file)

    def __init__(self, method: str = "lukas-kanade", **kwargs):
        super().__init__(method, **kwargs)

    def lk_kwargs(self) -> dict:
        """The keyword arguments of calc_optical_flow_lukas_kanade (cv.py:501-508)."""
        return dict(win_size=self.lk_window_size, max_level=self.lk_max_level, step=self.lk_step)


class LiteFlowNetConfig(MethodConfig):
    """The "liteflownet" method of CvFlowConfig (assets/configs/liteflownet.json: only the method key) and the weights
    that serve it: a path to the network's state dict or a dict of arrays (transflow_amd/liteflownet.py).  Other keys
    are carried in `.extra`; the weights never go into to_dict(), so no file alone makes this config (no from_file)."""

    METHOD = "liteflownet"
    HIP_KEYS = ("hip_lfn_precision",)

    def __init__(self, method: str = "liteflownet", weights=None, **kwargs):
        if method == self.METHOD and weights is None:
            raise ValueError("LiteFlowNetConfig needs the network's weights (a path or a dict of arrays)")
        super().__init__(method, **kwargs)
        self.weights = weights

    @classmethod
    def from_reference(cls, cfg, weights):
        return super().from_reference(cfg, weights=weights)


# The flow methods this backend serves: CvFlowSource.Method's name -> (the config class, the keyword argument of the
# readers below that opts the method in (None: served as it is), how the refusal without it shows that keyword, the
# constructor argument the opt-in's value becomes (None: it only switches)).
METHODS = {
    "farneback": (FlowConfig, None, None, None),
    "horn-schunck": (HornSchunckConfig, None, None, None),
    "lukas-kanade": (LucasKanadeConfig, "lucas_kanade", "lucas_kanade=True", None),
    "liteflownet": (LiteFlowNetConfig, "liteflownet", "liteflownet=<weights>", "weights"),
}
CONFIG_CLASSES = tuple(row[0] for row in METHODS.values())


def _method_name(method) -> str:
    """A method given as the reference's enum (CvFlowSource.Method) or as its string."""
    if method is None:
        return "farneback"
    if isinstance(method, str):
        return method.lower().strip()
    name = getattr(method, "name", str(method)).lower()
    return name.replace("_", "-")


def _serving(method, lucas_kanade, liteflownet):
    """METHODS' row for a method as a reader needs it: (name or None, config class, constructor arguments from the
    opt-in).  ValueError for a method whose opt-in was not given.  A name the table does not hold goes to FlowConfig
    as it came (name None)."""
    name = _method_name(method)
    if name not in METHODS:
        return None, FlowConfig, {}
    cls, opt_in, shown, becomes = METHODS[name]
    value = {"lucas_kanade": lucas_kanade or None, "liteflownet": liteflownet}.get(opt_in)
    if opt_in is not None and value is None:
        raise ValueError(f"transflow_amd does not implement the {name!r} flow method ({shown} serves it)")
    return name, cls, ({becomes: value} if becomes else {})


def flow_config_from_dict(d: dict, lucas_kanade: bool = False, liteflownet=None):
    """liteflownet: the network's weights (a path or a dict of arrays); with them a "liteflownet" config is served."""
    name, cls, given = _serving(d.get("method", "farneback"), lucas_kanade, liteflownet)
    if name in (None, "farneback"):
        return cls(**d)             # (the method as the file spells it: FlowConfig refuses what is not "farneback")
    return cls(**{**d, "method": name, **given})


def flow_config_from_file(path: str, lucas_kanade: bool = False, liteflownet=None):
    """A CvFlowConfig JSON file -> FlowConfig (farneback), HornSchunckConfig, LucasKanadeConfig when lucas_kanade
    is true, or LiteFlowNetConfig when liteflownet (the weights) is given; ValueError for the methods this backend
    does not compute (lukas-kanade and liteflownet by default) and for unknown ones."""
    with open(path, "r", encoding="utf8") as f:
        return flow_config_from_dict(json.load(f), lucas_kanade=lucas_kanade, liteflownet=liteflownet)


def flow_config_from_reference(cfg, lucas_kanade: bool = False, liteflownet=None):
    """A reference CvFlowConfig object (or one of ours, or None) -> FlowConfig, HornSchunckConfig, (lucas_kanade)
    LucasKanadeConfig or (liteflownet weights) LiteFlowNetConfig, by its method."""
    if isinstance(cfg, CONFIG_CLASSES):
        return cfg
    _, cls, given = _serving(getattr(cfg, "method", None), lucas_kanade, liteflownet)
    return cls.from_reference(cfg, **given)


def flow_config_from_arg(cv_config, lucas_kanade: bool = False, liteflownet=None):
    """The `cv_config` argument of FlowSource.from_args (source.py:365-411): a JSON path (the defaults when there is
    no such file, source.py:405-410), a CvFlowConfig object, one of ours, or None."""
    if isinstance(cv_config, str):
        if not os.path.isfile(cv_config):
            return FlowConfig()
        return flow_config_from_file(cv_config, lucas_kanade=lucas_kanade, liteflownet=liteflownet)
    return flow_config_from_reference(cv_config, lucas_kanade=lucas_kanade, liteflownet=liteflownet)
