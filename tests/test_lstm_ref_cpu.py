"""CPU: tests/lstm_ref.py, the reference tests/test_gpu_lstm.py holds the LSTM kernels and the timestamp head's tail to, against
two independent statements of the same arithmetic: torch.nn.LSTM in float64 (gate order, bias placement, the reverse direction,
stacking) and Oracle.us_alphas_peak's renormalisation and integrator."""
import numpy as np
import torch

import lstm_ref as LR
from aliparaformerasr_amd import weights as W
from oracle import model as om

D = 512


def _params(rng, n, scale=1.0):
    """n sets of (w_ih [4D, In], w_hh [4D, D], b_ih, b_hh) float64, In = D"""
    return [(rng.standard_normal((4 * D, D)) / np.sqrt(D), scale * rng.standard_normal((4 * D, D)) / np.sqrt(D),
             0.1 * rng.standard_normal(4 * D), 0.1 * rng.standard_normal(4 * D)) for _ in range(n)]


def _load(lstm, sets, names):
    with torch.no_grad():
        for (wih, whh, bih, bhh), sfx in zip(sets, names):
            getattr(lstm, "weight_ih_" + sfx).copy_(torch.from_numpy(wih))
            getattr(lstm, "weight_hh_" + sfx).copy_(torch.from_numpy(whh))
            getattr(lstm, "bias_ih_" + sfx).copy_(torch.from_numpy(bih))
            getattr(lstm, "bias_hh_" + sfx).copy_(torch.from_numpy(bhh))


def test_exact_float64_is_torch_lstm_bidirectional():
    rng = np.random.default_rng(1)
    B, T3 = 3, 7
    sets = _params(rng, 2, scale=2.0)
    x = rng.standard_normal((B, T3, D))
    lstm = torch.nn.LSTM(D, D, batch_first=True, bidirectional=True).double()
    _load(lstm, sets, ("l0", "l0_reverse"))
    with torch.no_grad():
        want = lstm(torch.from_numpy(x))[0].numpy()
    xg = np.concatenate([x @ wih.T + bih + bhh for wih, _, bih, bhh in sets], axis=-1)      # the input GEMM is the caller's
    got = LR.lstm_ref(xg, np.stack([s[1] for s in sets]), 2, np.float64, "exact")
    assert got.shape == want.shape == (B, T3, 2 * D)
    assert np.abs(got - want).max() < 1e-12


def test_exact_float64_is_torch_lstm_two_stacked_layers():
    """The hot-word embedder's shape class: forward only, layer 2 reads layer 1's hidden sequence."""
    rng = np.random.default_rng(2)
    B, T3 = 4, 6
    sets = _params(rng, 2)
    x = rng.standard_normal((B, T3, D))
    lstm = torch.nn.LSTM(D, D, num_layers=2, batch_first=True).double()
    _load(lstm, sets, ("l0", "l1"))
    with torch.no_grad():
        want = lstm(torch.from_numpy(x))[0].numpy()
    cur = x
    for wih, whh, bih, bhh in sets:
        cur = LR.lstm_ref(cur @ wih.T + bih + bhh, whh[None], 1, np.float64, "exact")
    assert np.abs(cur - want).max() < 1e-12


def test_operand_rounding_is_applied_to_the_recurrent_product_only():
    rng = np.random.default_rng(3)
    x = rng.standard_normal(4096).astype(np.float32)
    f16 = LR.round_operand(x, "f16", np.float64)
    pair = LR.round_operand(x, "pair", np.float64)
    assert np.array_equal(f16, x.astype(np.float16).astype(np.float64))
    assert np.abs(f16 - x).max() > 1e-4                                  # 11 bits
    assert np.abs(pair - x).max() < np.abs(x).max() * 2.0 ** -21        # 22 bits
    assert np.array_equal(LR.round_operand(x, "pair", np.float32).astype(np.float64), pair)
    # W_hh = 0: the recurrent product vanishes and every operand mode gives the same cell, with xg untouched by any rounding
    xg = rng.standard_normal((2, 3, 4 * D)).astype(np.float32)
    z = np.zeros((1, 4 * D, D), np.float32)
    a = LR.lstm_ref(xg, z, 1, np.float64, "exact")
    for mode in ("f16", "pair"):
        assert np.array_equal(LR.lstm_ref(xg, z, 1, np.float64, mode), a)
    # and the modes differ once W_hh is there, each by its own precision
    w = (rng.standard_normal((1, 4 * D, D)) / np.sqrt(D)).astype(np.float32)
    e = LR.lstm_ref(xg, w, 1, np.float64, "exact")
    d16 = np.abs(LR.lstm_ref(xg, w, 1, np.float64, "f16") - e).max()
    dpair = np.abs(LR.lstm_ref(xg, w, 1, np.float64, "pair") - e).max()
    assert 1e-6 < d16 < 1e-3 and dpair < d16 / 256, (d16, dpair)


def test_stale_hook_moves_the_hidden_sequence():
    rng = np.random.default_rng(4)
    xg = rng.standard_normal((2, 5, 8 * D)).astype(np.float32)
    w = (rng.standard_normal((2, 4 * D, D)) / np.sqrt(D)).astype(np.float32)
    a = LR.lstm_ref(xg, w, 2, np.float64, "f16")
    b = LR.lstm_ref(xg, w, 2, np.float64, "f16", hook=LR.stale_units(np.arange(8, 16)))
    # forward: frames 0 and 1 read h_{-1} = 0 and h_0 with or without the hook's shift of h_{-2} = h_{-1} = 0 -> frame 0 equal
    assert np.array_equal(a[:, 0, :D], b[:, 0, :D]) and np.array_equal(a[:, -1, D:], b[:, -1, D:])
    assert np.abs(a - b).max() > 1e-3


def _oracle():
    cfg = W.seaco_paraformer_config(enc_layers=0, dec_layers=0, seaco_layers=0, seaco_lstm_layers=1, vocab=16)
    return cfg, om.Oracle(om.ModelConfig(**cfg), W.synth_weights(cfg, seed=5), quant="fp32")


def test_us_peak_ref_is_the_oracles_last_two_stages():
    cfg, orc = _oracle()
    rng = np.random.default_rng(6)
    B, T = 5, 23
    H = torch.from_numpy(rng.standard_normal((B, T, D)).astype(np.float32))
    token_num = np.asarray([0, 1, 7, 30, 3], np.int32)                   # 30: above the raw sum, the renormalisation scales up
    seen = []
    tail = orc.us_renorm_peak
    orc.us_renorm_peak = lambda a2, tn: (seen.append(a2.copy()), tail(a2, tn))[1]
    want_a, want_p = orc.us_alphas_peak(H, token_num)
    raw = seen[0]
    assert raw.shape == (B, 3 * T) and raw.dtype == np.float32 and (raw.sum(axis=1) > 0).all() and raw.sum(axis=1).max() < 30
    thr = np.float32(np.float32(cfg["cif_threshold"]) - np.float32(1e-4))
    # the integrator alone, on the oracle's renormalised alphas: bit for bit
    assert np.array_equal(LR.cif_integrate_ref(want_a, thr), want_p)
    assert (want_p[3] >= thr).sum() >= 25 and (np.diff(np.flatnonzero(want_p[3] >= thr)) == 1).any()   # fires in consecutive frames
    # renormalisation: the oracle sums in float32 (numpy's pairwise order), us_peak_ref in float64 rounded once, as the kernel.
    # Rows where the two sums are the same float32 must agree bit for bit through both stages; the rest differ by that one ulp
    got_a, got_p = LR.us_peak_ref(raw, token_num, thr)
    same = LR.us_sums(raw)[0] == raw.sum(axis=1, dtype=np.float32)
    assert same.sum() >= 3, same
    assert np.array_equal(got_a[same], want_a[same]) and np.array_equal(got_p[same], want_p[same])
    assert np.abs(got_a - want_a).max() <= 2.0 ** -22 * np.abs(want_a).max()
    assert np.array_equal(got_a[0], np.zeros(3 * T, np.float32)) and np.array_equal(got_p[0], np.zeros(3 * T, np.float32))


def test_us_sums_orders():
    rng = np.random.default_rng(7)
    a = rng.random((6, 300), dtype=np.float32)
    seq, tree = LR.us_sums(a)
    exact = a.astype(np.float64).sum(axis=1)
    assert np.abs(seq - exact).max() <= 2.0 ** -24 * exact.max() * 1.01 and np.abs(tree - exact).max() <= 2.0 ** -24 * exact.max() * 1.01
    # T3 < 64: lanes past the row hold 0 and the tree still adds every element once
    s1, t1 = LR.us_sums(a[:, :5])
    assert np.array_equal(s1, t1) or np.abs(s1 - t1).max() < 1e-6
    assert np.allclose(t1, a[:, :5].astype(np.float64).sum(axis=1), rtol=1e-7)


def test_us_alpha_ref_is_the_oracles_formula():
    cfg, orc = _oracle()
    rng = np.random.default_rng(8)
    h = rng.uniform(-1, 1, (7, 2 * D)).astype(np.float32)
    w = orc.w["predictor.out2.weight"].numpy().reshape(-1)
    b0 = float(orc.w["predictor.out2.bias"].numpy()[0])
    z = torch.matmul(torch.from_numpy(h).double(), torch.from_numpy(w).double()) + b0
    want = torch.relu(torch.sigmoid(z) * cfg["cif_smooth2"] - cfg["cif_noise2"]).numpy()
    got = LR.us_alpha_ref(h, w, b0, cfg["cif_smooth2"], cfg["cif_noise2"])
    assert got.dtype == np.float64 and np.abs(got - want).max() < 1e-15
    assert LR.us_alpha_ref(h, w, b0, cfg["cif_smooth2"], cfg["cif_noise2"], np.float32).dtype == np.float32
