"""Parameter objects of the hot path, mirroring the reference's own
(same names, defaults and parsing), so a config built for transflow drives this
backend unchanged.

  LayerConfig   <- transflow/config.py:57-104   (fields the compositor reads)
  FlowConfig    <- CvFlowConfig, transflow/flow/sources/cv.py:271-363 (the fb_* fields)
  HornSchunckConfig <- the same, method "horn-schunck" (the hs_* fields)
  LucasKanadeConfig <- the same, method "lukas-kanade" (the lk_* fields; opt-in: lucas_kanade=True)
  LiteFlowNetConfig <- the same, method "liteflownet" (no fields; opt-in: liteflownet=<weights path or dict>)
"""
from __future__ import annotations

import json

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


class FlowConfig:
    """The Farnebäck fields of CvFlowConfig (cv.py:273-281) and their defaults; other
    methods' fields (hs_*, lk_*) are accepted and carried so a CvFlowConfig JSON loads."""

    FB_DEFAULTS = dict(fb_pyr_scale=0.5, fb_levels=3, fb_winsize=15, fb_iterations=3, fb_poly_n=5,
                       fb_poly_sigma=1.2, fb_flags=0)

    def __init__(self, method: str = "farneback", **kwargs):
        if method != "farneback":
            raise ValueError(f"transflow_amd implements the 'farneback' method only, got {method!r}")
        self.method = method
        for k, v in self.FB_DEFAULTS.items():
            setattr(self, k, kwargs.pop(k, v))
        # This backend's own key in a CvFlowConfig JSON: "hip_exact_sums": true asks for the box window summed in
        # OpenCV's own order (library option fb_exact_sums: flows bit-identical to the CPU path's, about 1.5 times
        # the Farnebäck time for a single 4K pair).  The reference ignores keys it does not know only if they are not there: leave it out
        # of files the reference itself must read.
        self.hip_exact_sums = parse_bool_arg(kwargs.pop("hip_exact_sums", None), False)
        # "hip_prefetch": n > 0 lets the flow source run up to n flows ahead of its consumer in a worker thread with a
        # library stream of its own (what the reference gets from running the source in a child process behind a
        # queue, pipeline.py:56-64, for a source used in-process).  Its position attributes then run ahead by as much.
        self.hip_prefetch = int(kwargs.pop("hip_prefetch", 0) or 0)
        # "hip_device_flows": true -- the source yields DeviceFlow objects (transflow_amd/deviceflow.py): flows that stay in
        # HBM until something reads them on the host, and that HipCompositor.update takes by device address (no 66 MB per
        # 4K frame down the link and up again across pipeline.py:562-567).  "ipc": the same, and through a multiprocessing
        # queue (pipeline.py:85-86) such a flow travels as a 64-byte HIP IPC handle instead of the pickled array.
        # "hip_batch": n > 1 -- where nothing can look at a raw flow in between (no lock expressions, no convolution kernel,
        # no initial flow), the source reads n frames ahead and computes their n pairs in ONE Farneback call: a single 4K
        # pair leaves most of the chip idle at the coarse levels, a batch of four costs 0.6 of four single calls.  Flows
        # still come out one at a time, in order, each post-processed with its own t.
        self.hip_batch = max(1, int(kwargs.pop("hip_batch", 1) or 1))
        v = kwargs.pop("hip_device_flows", None)
        self.hip_device_flows = "ipc" if isinstance(v, str) and v.lower() == "ipc" else parse_bool_arg(v, False)
        self.extra = dict(kwargs)  # hs_*, lk_*, show_window ...: not used by this backend

    def fb_kwargs(self) -> dict:
        return dict(pyr_scale=self.fb_pyr_scale, levels=self.fb_levels, winsize=self.fb_winsize,
                    iterations=self.fb_iterations, poly_n=self.fb_poly_n, poly_sigma=self.fb_poly_sigma,
                    flags=self.fb_flags)

    def to_dict(self) -> dict:
        d = {"method": self.method}
        d.update({k: getattr(self, k) for k in self.FB_DEFAULTS})
        d.update(self.extra)
        if self.hip_exact_sums:
            d["hip_exact_sums"] = True
        if self.hip_prefetch:
            d["hip_prefetch"] = self.hip_prefetch
        if self.hip_device_flows:
            d["hip_device_flows"] = self.hip_device_flows
        if self.hip_batch > 1:
            d["hip_batch"] = self.hip_batch
        return d

    def to_file(self, path: str):
        with open(path, "w", encoding="utf8") as f:
            json.dump(self.to_dict(), f, indent=4)

    @classmethod
    def from_file(cls, path: str):
        with open(path, "r", encoding="utf8") as f:
            return cls(**json.load(f))

    @classmethod
    def from_reference(cls, cfg):
        if cfg is None:
            return cls()
        if isinstance(cfg, cls):
            return cfg
        return cls(**{k: getattr(cfg, k) for k in cls.FB_DEFAULTS if hasattr(cfg, k)})


class HornSchunckConfig:
    """The Horn-Schunck fields of CvFlowConfig (cv.py:282-285) and their defaults; `hs_delta` may be None (JSON null:
    every call runs hs_iterations iterations).  fb_*, lk_* and other keys are carried in `.extra`."""

    HS_DEFAULTS = dict(hs_alpha=1, hs_iterations=3, hs_decay=0, hs_delta=1)
    # this backend's keys that Horn-Schunck has no use for (they shape the Farnebäck path)
    _FB_ONLY_HIP = ("hip_exact_sums", "hip_batch", "hip_device_flows")

    def __init__(self, method: str = "horn-schunck", **kwargs):
        if method != "horn-schunck":
            raise ValueError(f"HornSchunckConfig is the 'horn-schunck' method, got {method!r}")
        self.method = method
        for k, v in self.HS_DEFAULTS.items():
            setattr(self, k, kwargs.pop(k, v))
        for k in list(kwargs):
            if k.startswith("hip_") and k != "hip_prefetch":
                raise ValueError(f"{k!r} is not available with the horn-schunck method (only 'hip_prefetch' is)")
        # "hip_prefetch": as FlowConfig's
        self.hip_prefetch = int(kwargs.pop("hip_prefetch", 0) or 0)
        self.extra = dict(kwargs)

    def hs_kwargs(self) -> dict:
        """The keyword arguments of calc_optical_flow_horn_schunck (cv.py:495-498)."""
        return dict(alpha=self.hs_alpha, max_iters=self.hs_iterations, decay=self.hs_decay, delta=self.hs_delta)

    def to_dict(self) -> dict:
        d = {"method": self.method}
        d.update({k: getattr(self, k) for k in self.HS_DEFAULTS})
        d.update(self.extra)
        if self.hip_prefetch:
            d["hip_prefetch"] = self.hip_prefetch
        return d

    def to_file(self, path: str):
        with open(path, "w", encoding="utf8") as f:
            json.dump(self.to_dict(), f, indent=4)

    @classmethod
    def from_file(cls, path: str):
        with open(path, "r", encoding="utf8") as f:
            return cls(**json.load(f))

    @classmethod
    def from_reference(cls, cfg):
        if isinstance(cfg, cls):
            return cfg
        return cls(**{k: getattr(cfg, k) for k in cls.HS_DEFAULTS if hasattr(cfg, k)})


class LucasKanadeConfig:
    """The Lucas-Kanade fields of CvFlowConfig and their defaults (lk_window_size 15, lk_max_level 2, lk_step 1).
    fb_*, hs_* and other keys are carried in `.extra`."""

    LK_DEFAULTS = dict(lk_window_size=15, lk_max_level=2, lk_step=1)

    def __init__(self, method: str = "lukas-kanade", **kwargs):
        if method != "lukas-kanade":
            raise ValueError(f"LucasKanadeConfig is the 'lukas-kanade' method, got {method!r}")
        self.method = method
        for k, v in self.LK_DEFAULTS.items():
            setattr(self, k, kwargs.pop(k, v))
        for k in list(kwargs):
            if k.startswith("hip_") and k != "hip_prefetch":
                raise ValueError(f"{k!r} is not available with the lukas-kanade method (only 'hip_prefetch' is)")
        self.hip_prefetch = int(kwargs.pop("hip_prefetch", 0) or 0)
        self.extra = dict(kwargs)

    def lk_kwargs(self) -> dict:
        """The keyword arguments of calc_optical_flow_lukas_kanade (cv.py:501-508)."""
        return dict(win_size=self.lk_window_size, max_level=self.lk_max_level, step=self.lk_step)

    def to_dict(self) -> dict:
        d = {"method": self.method}
        d.update({k: getattr(self, k) for k in self.LK_DEFAULTS})
        d.update(self.extra)
        if self.hip_prefetch:
            d["hip_prefetch"] = self.hip_prefetch
        return d

    def to_file(self, path: str):
        with open(path, "w", encoding="utf8") as f:
            json.dump(self.to_dict(), f, indent=4)

    @classmethod
    def from_file(cls, path: str):
        with open(path, "r", encoding="utf8") as f:
            return cls(**json.load(f))

    @classmethod
    def from_reference(cls, cfg):
        if isinstance(cfg, cls):
            return cfg
        return cls(**{k: getattr(cfg, k) for k in cls.LK_DEFAULTS if hasattr(cfg, k)})


class LiteFlowNetConfig:
    """The "liteflownet" method of CvFlowConfig (assets/configs/liteflownet.json: only the method key) and the weights
    that serve it: a path to the network's state dict or a dict of arrays (transflow_amd/liteflownet.py).  Other keys
    are carried in `.extra`; the weights never go into to_dict()."""

    def __init__(self, method: str = "liteflownet", weights=None, **kwargs):
        if method != "liteflownet":
            raise ValueError(f"LiteFlowNetConfig is the 'liteflownet' method, got {method!r}")
        if weights is None:
            raise ValueError("LiteFlowNetConfig needs the network's weights (a path or a dict of arrays)")
        self.method = method
        self.weights = weights
        for k in list(kwargs):
            if k.startswith("hip_"):
                raise ValueError(f"{k!r} is not available with the liteflownet method")
        self.extra = dict(kwargs)

    def to_dict(self) -> dict:
        d = {"method": self.method}
        d.update(self.extra)
        return d

    def to_file(self, path: str):
        with open(path, "w", encoding="utf8") as f:
            json.dump(self.to_dict(), f, indent=4)

    @classmethod
    def from_reference(cls, cfg, weights):
        if isinstance(cfg, cls):
            return cfg
        return cls(weights=weights)


_UNSERVED_METHODS = ("lukas-kanade", "liteflownet")   # CvFlowSource.Method names this backend does not compute by default


def _method_name(method) -> str:
    """A method given as the reference's enum (CvFlowSource.Method) or as its string."""
    if method is None:
        return "farneback"
    if isinstance(method, str):
        return method.lower().strip()
    name = getattr(method, "name", str(method)).lower()
    return name.replace("_", "-")


def _refuse(method: str, lucas_kanade: bool, liteflownet=None) -> None:
    if method == "lukas-kanade" and lucas_kanade:
        return
    if method == "liteflownet" and liteflownet is not None:
        return
    if method in _UNSERVED_METHODS:
        hint = {"lukas-kanade": " (lucas_kanade=True serves it)",
                "liteflownet": " (liteflownet=<weights> serves it)"}.get(method, "")
        raise ValueError(f"transflow_amd does not implement the {method!r} flow method{hint}")


def flow_config_from_dict(d: dict, lucas_kanade: bool = False, liteflownet=None):
    """liteflownet: the network's weights (a path or a dict of arrays); with them a "liteflownet" config is served."""
    method = _method_name(d.get("method", "farneback"))
    _refuse(method, lucas_kanade, liteflownet)
    if method == "liteflownet":
        return LiteFlowNetConfig(**{**d, "method": method, "weights": liteflownet})
    if method == "lukas-kanade":
        return LucasKanadeConfig(**{**d, "method": method})
    if method == "horn-schunck":
        return HornSchunckConfig(**{**d, "method": method})
    return FlowConfig(**d)


def flow_config_from_file(path: str, lucas_kanade: bool = False, liteflownet=None):
    """A CvFlowConfig JSON file -> FlowConfig (farneback), HornSchunckConfig, LucasKanadeConfig when lucas_kanade
    is true, or LiteFlowNetConfig when liteflownet (the weights) is given; ValueError for the methods this backend
    does not compute (lukas-kanade and liteflownet by default) and for unknown ones."""
    with open(path, "r", encoding="utf8") as f:
        return flow_config_from_dict(json.load(f), lucas_kanade=lucas_kanade, liteflownet=liteflownet)


def flow_config_from_reference(cfg, lucas_kanade: bool = False, liteflownet=None):
    """A reference CvFlowConfig object (or one of ours, or None) -> FlowConfig, HornSchunckConfig, (lucas_kanade)
    LucasKanadeConfig or (liteflownet weights) LiteFlowNetConfig, by its method."""
    if cfg is None:
        return FlowConfig()
    if isinstance(cfg, (FlowConfig, HornSchunckConfig, LucasKanadeConfig, LiteFlowNetConfig)):
        return cfg
    method = _method_name(getattr(cfg, "method", None))
    _refuse(method, lucas_kanade, liteflownet)
    if method == "liteflownet":
        return LiteFlowNetConfig.from_reference(cfg, liteflownet)
    if method == "lukas-kanade":
        return LucasKanadeConfig.from_reference(cfg)
    if method == "horn-schunck":
        return HornSchunckConfig.from_reference(cfg)
    return FlowConfig.from_reference(cfg)
