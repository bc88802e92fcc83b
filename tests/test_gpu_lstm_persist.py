"""Persistent large-H recurrence (one cooperative launch per layer, W_hh
register-resident, per-batch-block grid sync; csrc/kernels/lstm_large.hip)
against the per-step MFMA kernels on identical inputs, and the char-LM-shaped
layer against the fp32 torch reference.  PDRNN_LSTM_PERSIST_CHECK=1
(conftest) makes every persistent launch check its sync-timeout flag."""
import pytest
import torch

from pytorch_distributed_rnn_amd import _ext
from pytorch_distributed_rnn_amd.models.rnn import LSTM

pytestmark = pytest.mark.gpu

H = 1024


def _rel(a, b):
    return float((a.float() - b.float()).norm() / (b.float().norm() + 1e-12))


def _run(mod, tile, xp, w, wt, h0, c0, dout, dhn, dcn, rev, cell):
    hseq, cseq, acts = mod.lstm_large_fwd(xp, w, h0, c0, H, rev, tile, cell)
    dg, dh0, dc0 = mod.lstm_large_bwd(dout, dhn, dcn, wt, cseq, acts, c0, H, rev, tile, cell)
    return hseq, cseq, acts, dg, dh0, dc0


@pytest.mark.parametrize("cell", [0, 1])
@pytest.mark.parametrize("B,T,ndir,rev", [(128, 9, 1, 0),    # char-LM shape: 256 workgroups, 16 rows each
                                          (200, 5, 1, 0),    # 2 x 16 rows per workgroup, clamped last block
                                          (40, 6, 2, 2),     # bidirectional, reverse direction 1
                                          (7, 4, 1, 1)])     # tiny batch, reversed
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_persistent_matches_per_step(cell, B, T, ndir, rev, dt):
    mod = _ext.require()
    assert mod.lstm_large_persist_mt(B, H, ndir, 0 if dt == torch.bfloat16 else 1) > 0
    torch.manual_seed(B + T + cell)
    dev = "cuda"
    xp = (torch.randn(T, B, ndir * 4 * H, device=dev) * 0.5).to(dt)
    w = [(torch.randn(4 * H, H, device=dev) * 0.03).to(dt) for _ in range(ndir)]
    wt = [(torch.randn(H, 4 * H, device=dev) * 0.03).to(dt) for _ in range(ndir)]
    h0 = (torch.randn(ndir, B, H, device=dev) * 0.5).to(dt)
    c0 = torch.randn(ndir, B, H, device=dev) * 0.5
    dout = (torch.randn(T, B, ndir * H, device=dev) * 0.1).to(dt)
    dhn = torch.randn(ndir, B, H, device=dev) * 0.1
    dcn = torch.randn(ndir, B, H, device=dev) * 0.1
    args = (xp, w, wt, h0, c0, dout, dhn, dcn, rev, cell)
    got = _run(mod, -1, *args)
    ref = _run(mod, 0, *args)
    torch.cuda.synchronize()
    names = ["hseq", "cseq", "acts", "dgates", "dh0", "dc0"][:6 if cell == 0 else 5]  # GRU: no dc0
    for name, a, b in zip(names, got, ref):
        assert torch.isfinite(a.float()).all(), name
        assert _rel(a, b) < 1e-2, (name, _rel(a, b))


@pytest.mark.parametrize("cell", [0, 1])
@pytest.mark.parametrize("Hs,B,T,ndir,rev", [(128, 1440, 6, 1, 0),  # motion --hidden-units 128 batch
                                             (128, 200, 5, 1, 0),   # last row block partial
                                             (128, 40, 6, 2, 2),
                                             (128, 7, 1, 2, 1),     # T = 1, one partial block
                                             (256, 7, 4, 1, 1),
                                             (256, 300, 3, 2, 0)])
def test_persistent_fp32_matches_per_step(cell, Hs, B, T, ndir, rev):
    """fp32 storage (the reference's precision at --hidden-units 128 / 256)
    on v_mfma_f32_16x16x4_f32 equals the per-step kernels up to fp32
    summation order: at H = 128 the row-owning recurrence
    (kernels/lstm_rows_f32.hip, forward and backward), at H = 256 the
    persistent backward (the fp32 forward runs the per-step kernels: its
    persistent form was slower and is not offered)."""
    mod = _ext.require()
    assert Hs == 128 or mod.lstm_large_persist_mt(B, Hs, ndir, 2) > 0
    torch.manual_seed(B + T + cell + Hs)
    dev = "cuda"
    xp = torch.randn(T, B, ndir * 4 * Hs, device=dev) * 0.5
    w = [torch.randn(4 * Hs, Hs, device=dev) * 0.06 for _ in range(ndir)]
    wt = [torch.randn(Hs, 4 * Hs, device=dev) * 0.06 for _ in range(ndir)]
    h0 = torch.randn(ndir, B, Hs, device=dev) * 0.5
    c0 = torch.randn(ndir, B, Hs, device=dev) * 0.5
    dout = torch.randn(T, B, ndir * Hs, device=dev) * 0.1
    dhn = torch.randn(ndir, B, Hs, device=dev) * 0.1
    dcn = torch.randn(ndir, B, Hs, device=dev) * 0.1

    def run(tile):
        hseq, cseq, acts = mod.lstm_large_fwd(xp, w, h0, c0, Hs, rev, tile, cell)
        dg, dh0, dc0 = mod.lstm_large_bwd(dout, dhn, dcn, wt, cseq, acts, c0, Hs, rev, tile, cell)
        return hseq, cseq, acts, dg, dh0, dc0
    got, ref = run(-1), run(0)
    torch.cuda.synchronize()
    names = ["hseq", "cseq", "acts", "dgates", "dh0", "dc0"][:6 if cell == 0 else 5]
    for name, a, b in zip(names, got, ref):
        assert torch.isfinite(a).all(), name
        assert _rel(a, b) < 1e-5, (name, _rel(a, b))


def test_persistent_charlm_layer_matches_torch():
    """nn.LSTM(64 -> 1024) at the char-LM batch on the persistent path vs fp32 torch."""
    torch.manual_seed(5)
    dt = torch.bfloat16
    m = LSTM(64, H, 1, batch_first=True).cuda()
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(p.to(dt).float())
    ref = torch.nn.LSTM(64, H, 1, batch_first=True).cuda()
    with torch.no_grad():
        for (n, p), (_, q) in zip(m.named_parameters(), ref.named_parameters()):
            q.copy_(p)
    x = torch.randn(128, 24, 64, device="cuda").to(dt)
    x16 = x.clone().requires_grad_(True)
    xr = x.float().clone().requires_grad_(True)
    out, (hn, cn) = m(x16)
    out_r, (hn_r, cn_r) = ref(xr)
    assert _rel(out, out_r) < 2e-2 and _rel(cn, cn_r) < 2e-2
    g = torch.randn_like(out_r)
    (out.float() * g).sum().backward()
    (out_r * g).sum().backward()
    assert _rel(x16.grad, xr.grad) < 4e-2
    for (n, p), (_, q) in zip(m.named_parameters(), ref.named_parameters()):
        assert _rel(p.grad, q.grad) < 4e-2, n


def _inputs(B, T, ndir, dt, seed):
    torch.manual_seed(seed)
    dev = "cuda"
    xp = (torch.randn(T, B, ndir * 4 * H, device=dev) * 0.5).to(dt)
    w = [(torch.randn(4 * H, H, device=dev) * 0.03).to(dt) for _ in range(ndir)]
    wt = [(torch.randn(H, 4 * H, device=dev) * 0.03).to(dt) for _ in range(ndir)]
    h0 = (torch.randn(ndir, B, H, device=dev) * 0.5).to(dt)
    c0 = torch.randn(ndir, B, H, device=dev) * 0.5
    dout = (torch.randn(T, B, ndir * H, device=dev) * 0.1).to(dt)
    dhn = torch.randn(ndir, B, H, device=dev) * 0.1
    dcn = torch.randn(ndir, B, H, device=dev) * 0.1
    return xp, w, wt, h0, c0, dout, dhn, dcn


@pytest.fixture
def verified():
    mod = _ext.require()
    mod.set_persist_verify(1)
    mod.persist_reset()
    yield mod
    mod.set_persist_verify(0)
    mod.persist_inject_timeouts(0)
    mod.persist_reset()


def test_persistent_timeout_rerun_on_per_step_kernels(verified):
    """ADVICE r2 / VERDICT r2 item 2b: a persistent launch whose grid sync
    timed out (here: flagged by the kernel's test hook, waiters released
    early -- invalid outputs) is detected in the same call and the layer is
    re-run on the per-step kernels, so forward AND backward still equal the
    per-step path and nothing invalid reaches the caller."""
    mod = verified
    B, T, ndir, dt = 128, 9, 1, torch.bfloat16
    xp, w, wt, h0, c0, dout, dhn, dcn = _inputs(B, T, ndir, dt, 11)
    ref = _run(mod, 0, xp, w, wt, h0, c0, dout, dhn, dcn, 0, 0)
    before = mod.persist_fallbacks()
    mod.persist_inject_timeouts(1)  # the forward launch
    got = _run(mod, -1, xp, w, wt, h0, c0, dout, dhn, dcn, 0, 0)
    torch.cuda.synchronize()
    # one timed-out launch turns the persistent path off for the
    # process (the backward already runs on the per-step kernels) instead of
    # paying the 2 s spin bound again every step
    assert mod.persist_fallbacks() - before == 1 and mod.persist_disabled()
    for name, a, b in zip(["hseq", "cseq", "acts", "dgates", "dh0", "dc0"], got, ref):
        assert _rel(a, b) < 1e-2, (name, _rel(a, b))
    got2 = _run(mod, -1, xp, w, wt, h0, c0, dout, dhn, dcn, 0, 0)
    torch.cuda.synchronize()
    assert mod.persist_fallbacks() - before == 1
    for a, b in zip(got2, ref):
        assert _rel(a, b) < 1e-2
    # re-enabled (tests only), a clean launch takes the persistent path again
    mod.persist_reset()
    got3 = _run(mod, -1, xp, w, wt, h0, c0, dout, dhn, dcn, 0, 0)
    torch.cuda.synchronize()
    assert mod.persist_fallbacks() == 0 and not mod.persist_disabled()
    for a, b in zip(got3, ref):
        assert _rel(a, b) < 1e-2
    mod.persist_check()  # no sticky timeout left behind


def test_persistent_backward_beside_cu_spinner(verified):
    """The co-residency hazard itself: a side stream fills every CU with
    bounded spinning workgroups while the persistent backward launches.  The
    cooperative grid either waits for the CUs (no timeout) or loses
    co-residency, times out and is re-run -- either way the gradients equal
    the per-step path and no error is left sticky."""
    mod = verified
    B, T, ndir, dt = 128, 9, 1, torch.bfloat16
    xp, w, wt, h0, c0, dout, dhn, dcn = _inputs(B, T, ndir, dt, 12)
    hseq, cseq, acts = mod.lstm_large_fwd(xp, w, h0, c0, H, 0, 0, 0)
    ref = mod.lstm_large_bwd(dout, dhn, dcn, wt, cseq, acts, c0, H, 0, 0, 0)
    torch.cuda.synchronize()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    side = torch.cuda.Stream()
    before = mod.persist_fallbacks()
    with torch.cuda.stream(side):
        mod.debug_spin_cus(2500.0, cus * 2, 1024, 64 * 1024)  # 2 x (16 waves, 64 KB LDS) per CU, 2.5 s
    got = mod.lstm_large_bwd(dout, dhn, dcn, wt, cseq, acts, c0, H, 0, -1, 0)
    torch.cuda.synchronize()
    print("persistent fallbacks beside the spinner:", mod.persist_fallbacks() - before)
    for name, a, b in zip(["dgates", "dh0", "dc0"], got, ref):
        assert torch.isfinite(a.float()).all(), name
        assert _rel(a, b) < 1e-2, (name, _rel(a, b))
    mod.persist_check()


def test_step_verified_charlm_reruns_timed_out_step(monkeypatch):
    """ADVICE r3 / VERDICT r3 item 5a: per-step verification (the multi-rank
    default) without a host sync in the step: a timed-out persistent launch
    sets the device flag, the Adam launches of that step and of the next one
    (issued before the host saw the flag) skip themselves on the device, and
    the trainer re-runs both from the first one's carried state on the
    per-step kernels -- parameters and the returned losses equal a run that
    never took the persistent path."""
    import copy
    from pytorch_distributed_rnn_amd.data.charlm import CharCorpus
    from pytorch_distributed_rnn_amd.models.charlm import CharLM
    from pytorch_distributed_rnn_amd.train.lm import LMTrainer
    mod = _ext.require()
    if mod.lstm_large_persist_mt(16, 1024, 1, 0) == 0:
        pytest.skip("persistent recurrence not covered on this device")
    corpus = CharCorpus.synthetic(200_000, seed=3)
    torch.manual_seed(0)
    m0 = CharLM(256, 64, 1024, 1, compute_dtype=torch.bfloat16)
    results, losses = [], []
    try:
        for inject in (True, False):
            mod.persist_reset()
            mod.set_persist_verify(2 if inject else 0)
            if not inject:
                mod.persist_disable()  # reference run: per-step kernels only
            tr = LMTrainer(copy.deepcopy(m0), corpus, global_batch=16, seq_len=32, device=torch.device("cuda"))
            segs = list(CharCorpus.segments(tr.streams, 32, 3))
            tr.inner.reset_hidden_state()
            if inject:
                mod.persist_inject_timeouts(1)  # the first persistent launch of step 1
            out = [tr.train_step(inp, tgt) for inp, tgt in segs]
            tr.settle()
            torch.cuda.synchronize()
            if inject:
                assert mod.persist_fallbacks() == 1 and mod.persist_disabled()
                assert tr.optimizer._flat_state[0]["step"].item() == 3.0
            results.append(torch.cat([p.detach().float().reshape(-1) for p in tr.inner.parameters()]))
            losses.append(torch.stack(out).float())
    finally:
        mod.persist_inject_timeouts(0)
        mod.set_persist_verify(0)
        mod.persist_reset()
    torch.testing.assert_close(losses[0], losses[1], rtol=1e-3, atol=1e-5)
    torch.testing.assert_close(results[0], results[1], rtol=1e-3, atol=1e-5)
