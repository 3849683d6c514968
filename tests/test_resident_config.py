"""The `hip_resident` key of the flow configs (transflow_amd/config.py): parsing, round trips and what it opens."""
import json

import pytest

from transflow_amd.config import (FlowConfig, HornSchunckConfig, LiteFlowNetConfig, LucasKanadeConfig, flow_config_from_arg,
                                  flow_config_from_dict, flow_config_from_file)

THREE = [(HornSchunckConfig, {}, {}), (LucasKanadeConfig, {}, {"lucas_kanade": True}),
         (LiteFlowNetConfig, {"weights": "w.pt"}, {"liteflownet": "w.pt"})]


@pytest.mark.parametrize("cls,given,opt_in", THREE, ids=[c.METHOD for c, _, _ in THREE])
def test_keys_parse_and_round_trip(tmp_path, cls, given, opt_in):
    plain = cls(**given)
    assert plain.hip_resident is False and plain.hip_device_flows is False and plain.hip_batch == 1
    assert not any(k.startswith("hip_") for k in plain.to_dict())
    for value in (True, "yes", "1", 1):
        assert cls(hip_resident=value, **given).hip_resident is True
    for value in (False, "no", None, 0):
        assert cls(hip_resident=value, **given).hip_resident is False
    cfg = cls(hip_resident=True, hip_device_flows=True, hip_batch=3, **given)
    assert (cfg.hip_resident, cfg.hip_device_flows, cfg.hip_batch) == (True, True, 3)
    assert cls(hip_resident=True, hip_device_flows="ipc", **given).hip_device_flows == "ipc"
    d = cfg.to_dict()
    assert (d["hip_resident"], d["hip_device_flows"], d["hip_batch"]) == (True, True, 3) and "weights" not in d
    back = flow_config_from_dict(d, **opt_in)
    assert isinstance(back, cls) and back.to_dict() == d
    path = str(tmp_path / "cfg.json")
    cfg.to_file(path)
    assert json.load(open(path)) == d
    assert flow_config_from_file(path, **opt_in).to_dict() == d
    assert flow_config_from_arg(path, **opt_in).hip_resident is True
    only = cls(hip_resident=True, **given)
    assert only.to_dict()["hip_resident"] is True and "hip_batch" not in only.to_dict()
    assert (only.hip_device_flows, only.hip_batch) == (False, 1)


@pytest.mark.parametrize("cls,given,opt_in", THREE, ids=[c.METHOD for c, _, _ in THREE])
@pytest.mark.parametrize("key,value", [("hip_device_flows", True), ("hip_device_flows", "ipc"), ("hip_batch", 3)])
def test_resident_keys_need_the_switch(cls, given, opt_in, key, value):
    for switch in ({}, {"hip_resident": False}, {"hip_resident": "no"}):
        with pytest.raises(ValueError, match="hip_resident") as err:
            cls(**{key: value}, **switch, **given)
        assert key in str(err.value) and cls.METHOD in str(err.value)
    with pytest.raises(ValueError, match="hip_resident"):
        flow_config_from_dict({"method": cls.METHOD, key: value}, **opt_in)
    assert getattr(cls(**{key: value}, hip_resident=True, **given), key) == value


def test_farneback_config_is_unchanged_by_default():
    cfg = FlowConfig()
    assert cfg.hip_resident is False and "hip_resident" not in cfg.to_dict()
    assert cfg.to_dict() == {"method": "farneback", "fb_pyr_scale": 0.5, "fb_levels": 3, "fb_winsize": 15, "fb_iterations": 3,
                             "fb_poly_n": 5, "fb_poly_sigma": 1.2, "fb_flags": 0}
    assert (cfg.hip_exact_sums, cfg.hip_prefetch, cfg.hip_device_flows, cfg.hip_batch) == (False, 0, False, 1)
    assert FlowConfig(hip_device_flows=True, hip_batch=4).to_dict()["hip_batch"] == 4    # its own keys need no switch
    on = FlowConfig(fb_flags=4, hip_resident=True, hip_device_flows=True)
    assert on.hip_resident is True and on.extra == {} and on.to_dict()["hip_resident"] is True
    assert FlowConfig(**on.to_dict()).to_dict() == on.to_dict()


def test_sources_choose_their_route_by_the_key():
    """No GPU call: which route a source would take (HipFlowSource._resident_ok, _chains, _batch_size)."""
    import numpy as np

    from transflow_amd.flow import ArrayFrameProvider, HipFlowSource
    frames = [np.zeros((40, 48), np.uint8)] * 3

    def source(cfg, **kw):
        builder = HipFlowSource.from_args(ArrayFrameProvider(frames, 25.0), cv_config=cfg, **kw)
        builder.build()
        return builder.cls(*builder.args(), **builder.kwargs())
    s = source(HornSchunckConfig())
    assert not s._resident_ok() and s._chains() and s._batch_size() == 1
    s = source(HornSchunckConfig(hip_resident=True, hip_batch=4))
    assert s._resident_ok() and s._chains() and s._batch_size() == 1 and not s.chain_valid
    assert not source(HornSchunckConfig(hip_resident=True), lock_expr="1,1")._resident_ok()
    s = source(LucasKanadeConfig(hip_resident=True, hip_batch=4))
    assert s._resident_ok() and not s._chains() and s._batch_size() == 4
    assert not source(LucasKanadeConfig())._resident_ok()
    s = source(FlowConfig(hip_batch=4))                       # Farnebäck is resident as before, whatever the key says
    assert s._resident_ok() and s._own_tail() and s._batch_size() == 4
    assert source(FlowConfig(hip_resident=True))._own_tail()
    s = source(FlowConfig(fb_flags=4, hip_batch=4))
    assert not s._resident_ok() and s._batch_size() == 1
    s = source(FlowConfig(fb_flags=4, hip_resident=True, hip_batch=4))
    assert s._resident_ok() and s._chains() and not s._own_tail() and s._batch_size() == 1
