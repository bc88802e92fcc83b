"""The sequence-in-wave family's plan (pdrnn_lstm_sw_plan over the wave map
table of kernels/lstm_sw.hip): which map runs each pass of a batch, and the
launchers' refusal of a map the table does not list.  Host queries only."""
import copy

import pytest
import torch

from _tune import set_tune

pytestmark = pytest.mark.gpu

CUS = 256  # the plan is asked for an MI355X's 256 CUs (1024 SIMDs) whatever the device


def _mod():
    from pytorch_distributed_rnn_amd import _ext
    return _ext.native(torch.device("cuda", 0))


def _maps(NL, B, T=128):
    p = _mod().lstm_sw_plan(NL, B, T, cus=CUS)
    return p["fwd_map"], p["bwd_map"]


def test_sw_plan_table(monkeypatch):
    """Two layers: four waves per sequence + register dW in one launch up to
    two workgroups per CU (B <= 512), a wave per layer up to one wave per SIMD
    (1024), the chunked forward and the two-sequence backward above; the
    register-dW backward gives way to map 2 where T is no multiple of 4 and
    the chunked forward to map 6 where T is no whole number of 16-step chunks
    or its x rows (14,144 + 48 T bytes of LDS) do not let six workgroups share
    a CU (T > 256).  One layer: one sequence per wave up to one wave per SIMD,
    two above.  Overrides apply per pass, and only where the table lists the
    map for that pass and layer count."""
    mod = _mod()
    monkeypatch.delenv("PDRNN_SW", raising=False)
    set_tune(monkeypatch, sw_mode=None, sw_bwd_mode=None)
    for B in (97, 512):
        p = mod.lstm_sw_plan(2, B, 128, cus=CUS)
        assert p == {"fwd_map": 5, "bwd_map": 4, "fwd_nb": 1, "bwd_nb": 1, "one_launch": True, "register_dw": True}, (B, p)
    for B in (513, 1024):
        p = mod.lstm_sw_plan(2, B, 128, cus=CUS)
        assert p == {"fwd_map": 2, "bwd_map": 2, "fwd_nb": 1, "bwd_nb": 1, "one_launch": False, "register_dw": False}, (B, p)
    for B in (1025, 1440):
        p = mod.lstm_sw_plan(2, B, 128, cus=CUS)
        assert p == {"fwd_map": 8, "bwd_map": 3, "fwd_nb": 1, "bwd_nb": 2, "one_launch": False, "register_dw": False}, (B, p)
    p = mod.lstm_sw_plan(2, 180, 126, cus=CUS)
    assert (p["fwd_map"], p["bwd_map"], p["one_launch"], p["register_dw"]) == (5, 2, False, False), p
    for T, fwd in ((120, 6), (272, 6), (256, 8)):
        assert _maps(2, 1440, T) == (fwd, 3), T
    assert _maps(1, 1024) == (0, 0) and _maps(1, 1025) == (1, 1)
    assert mod.lstm_sw_plan(1, 1025, 128, cus=CUS)["fwd_nb"] == 2

    # the step's plan copies the family's (on the real device)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for B in (97, 2 * cus, 2 * cus + 1, 4 * cus, 4 * cus + 1, 1440):
        sp, hp = mod.lstm_sw_plan(2, B, 128), mod.lstm_head_step_plan(32, 9, 2, 128, B)
        assert hp["sw"] and (hp["sw_fmode"], hp["sw_bmode"], hp["sw_step"]) == (sp["fwd_map"], sp["bwd_map"], sp["one_launch"]), B
        assert hp["grid_dw"] == -(-B // sp["bwd_nb"]) and hp["stamps_fwd"][0] == -(-B // sp["fwd_nb"]), B
        assert hp["slab_rows"] == B or not sp["register_dw"], B  # register dW: a slab row per sequence
        assert mod.lstm_sw_step_ok(2, B, 128) == sp["one_launch"], B

    # overrides
    default = {B: mod.lstm_sw_plan(2, B, 128, cus=CUS) for B in (97, 720, 1440)}
    set_tune(monkeypatch, sw_mode="2")
    for B in default:
        assert _maps(2, B) == (2, 2), B  # sw_mode alone: both passes
    set_tune(monkeypatch, sw_mode="6")
    for B, d in default.items():
        assert _maps(2, B) == (6, d["bwd_map"]), B  # a forward map: the backward keeps the plan's
    set_tune(monkeypatch, sw_mode="3")
    for B, d in default.items():
        assert _maps(2, B) == (d["fwd_map"], 3), B  # a backward map: the forward keeps the plan's
    assert mod.lstm_sw_plan(2, 1440, 128, cus=CUS) == default[1440]
    set_tune(monkeypatch, sw_mode="0")  # one layer's map on two layers: ignored
    for B, d in default.items():
        assert mod.lstm_sw_plan(2, B, 128, cus=CUS) == d, B
    set_tune(monkeypatch, sw_mode=None, sw_bwd_mode="8")  # a forward map as the backward's: ignored
    for B, d in default.items():
        assert mod.lstm_sw_plan(2, B, 128, cus=CUS) == d, B
    set_tune(monkeypatch, sw_mode="2", sw_bwd_mode=None)  # a two-layer map on one layer: ignored
    assert _maps(1, 180) == (0, 0)
    set_tune(monkeypatch, sw_mode="8", sw_bwd_mode="4")  # forced maps still give way on T
    assert _maps(2, 1440, 126) == (6, 2) and _maps(2, 1440, 128) == (8, 4)


@pytest.mark.parametrize("NL,mode", [(2, 3), (2, 0), (1, 2), (2, 1), (2, 4), (2, 7), (1, 8), (2, -1), (2, 9)])
def test_forward_refuses_maps_the_table_does_not_list(NL, mode):
    """A backward-only map, one layer's maps on two layers, a two-layer map
    on one, and ids outside the table: pdrnn_lstm_sw_fwd returns
    hipErrorInvalidValue before anything is launched."""
    mod = _mod()
    torch.manual_seed(3)
    rnn = torch.nn.LSTM(9, 32, NL, batch_first=True).cuda()
    ws = [p.detach() for p in rnn.parameters()]
    x = torch.randn(2, 4, 9, device="cuda")
    with pytest.raises(RuntimeError):
        mod.lstm_sw_fwd(x, ws, 32, NL, mode)
    torch.cuda.synchronize()  # (nothing ran, nothing is pending)


def test_forward_serves_every_listed_map():
    """... and the same call goes through for each forward map of the table
    (map 8 at a whole chunk): same h_n from every two-layer map to fp32
    round-off, so the refusal above is the table's, not the shape's."""
    mod = _mod()
    torch.manual_seed(5)
    for NL, maps in ((1, (0, 1)), (2, (2, 5, 6, 8))):
        rnn = torch.nn.LSTM(9, 32, NL, batch_first=True).cuda()
        ws = [p.detach() for p in rnn.parameters()]
        x = torch.randn(3, 16, 9, device="cuda")
        with torch.no_grad():
            ref = copy.deepcopy(rnn).double()(x.double())[1][0]
        for m in maps:
            hn = mod.lstm_sw_fwd(x, ws, 32, NL, m)[2]
            assert (hn.double() - ref).abs().max().item() < 1e-5, (NL, m)
