"""GPU: the speaker clustering on the device (csrc/k_spk_cluster.hip; Engine.op_spk_cluster, OfflineRecognizer.SetSpeakerClustering)
against the host's walk (E.host_spk_cluster_trace, which tests/test_spk_cpu.py holds to the float64 definition) and, up to 150
windows, against the definition itself (spk_ref.cluster).  Labels, speaker counts and merge lists are compared as they are, the
merge heights by their bits: a fused product or a quotient rounded differently shows there and nowhere else."""
import ctypes as C
import functools

import numpy as np
import pytest

import spk_ref as R
from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd import engine as E
from test_gpu_spk import VAD_CFG, V_burst, _census, _segments, eng80, rec_paths  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

CONFIGS = [{}, dict(threshold=0.3, min_cluster=2), dict(num_speakers=3)]


@functools.lru_cache(maxsize=None)
def _cosines(n, seed=0):
    """fp32 cosines of n embeddings drawn around five centres (clusters of every size, so the averages' quotients are inexact)"""
    rng = np.random.default_rng(1000 * seed + n)
    centres = rng.standard_normal((5, 24))
    emb = centres[rng.integers(0, 5, n)] + 0.45 * rng.standard_normal((n, 24))
    S = R.affinity(emb).astype(np.float32).reshape(n, n)
    S.setflags(write=False)
    return S


def _check(eng, S_list, cfg):
    got = eng.op_spk_cluster(S_list, cfg)
    for S, (labels, k, merges, heights) in zip(S_list, got):
        h_labels, h_k, h_merges, h_heights = E.host_spk_cluster_trace(S, cfg)
        assert labels.tolist() == h_labels.tolist() and k == h_k
        assert merges.tolist() == h_merges.tolist()
        assert heights.view(np.uint64).tolist() == h_heights.view(np.uint64).tolist()
        if S.shape[0] <= 150:                                      # (pf_spk_config.threshold is a float: the definition gets that value)
            ref_labels, ref_k = R.cluster(S, **dict(cfg, threshold=float(np.float32(cfg.get("threshold", 0.5)))))
            assert labels.tolist() == ref_labels.tolist() and k == ref_k
    return got


@pytest.mark.parametrize("cfg", CONFIGS, ids=["default", "thr0.3_min2", "three"])
@pytest.mark.parametrize("n", [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2500])
def test_sizes_and_configs(n, cfg, eng80):
    (_, k, merges, _), = _check(eng80, [_cosines(n)], cfg)
    if n >= 63:                                                    # the case is one: clusters of odd sizes merged
        assert k < n and (merges >= 0).all(axis=1).sum() > n // 2


def _ties():
    return np.random.default_rng(5).choice(np.float32([0.25, 0.5, 0.75]), (96, 96))


def _planted():
    g = np.array([0] * 9 + [1] * 2 + [2] + [0] * 3 + [3] * 2 + [4] * 5)        # a cluster of 12, one of 5, minors of 2, 1, 2
    S = 0.1 + 0.8 * (g[:, None] == g[None, :]) + 0.05 * np.random.default_rng(6).random((g.size, g.size))
    return S.astype(np.float32)


def _not_finite():
    S = _cosines(50).copy()
    S[0, 1], S[2, 40], S[7, 8], S[20, 49] = np.nan, np.inf, -np.inf, np.nan
    return S


def _chain():
    i = np.arange(300)
    return (1.0 - np.abs(i[:, None] - i[None, :]) / 300.0).astype(np.float32)


CONSTRUCTED = {
    "ties": (_ties, [{}, dict(threshold=0.6, min_cluster=1)]),
    "all_equal_above": (lambda: np.full((130, 130), 0.8, np.float32), [{}]),
    "all_equal_below": (lambda: np.full((130, 130), 0.2, np.float32), [dict(min_cluster=4), dict(min_cluster=1)]),
    "planted_minors": (_planted, [{}, dict(min_cluster=3), dict(min_cluster=6)]),
    "num_speakers": (lambda: _cosines(40), [dict(num_speakers=1), dict(num_speakers=40), dict(num_speakers=100)]),
    "not_finite": (_not_finite, CONFIGS),
    "chain": (_chain, [{}, dict(num_speakers=1)]),
}


@pytest.mark.parametrize("name", list(CONSTRUCTED))
def test_constructed(name, eng80):
    make, cfgs = CONSTRUCTED[name]
    S = make()
    for cfg in cfgs:
        (labels, k, merges, _), = _check(eng80, [S], cfg)
        n_merges = int((merges >= 0).all(axis=1).sum())
        if name == "all_equal_above" or cfg.get("num_speakers") == 1:
            assert k == 1 and n_merges == S.shape[0] - 1
        if name == "all_equal_below":
            assert k == 130 and n_merges == 0 and labels.tolist() == list(range(130))
        if name == "planted_minors" and not cfg:
            assert k == 2 and set(labels.tolist()) == {0, 1}                          # the minors joined the major clusters


def test_lower_triangle_and_diagonal_are_not_read(eng80):
    S = _cosines(70)
    bad = np.triu(S, 1) + np.tril(1.0 - S.T, -1)                  # a lower triangle that contradicts the upper one
    bad[np.tril_indices(70, -1)[0][::3], np.tril_indices(70, -1)[1][::3]] = np.nan
    np.fill_diagonal(bad, np.nan)
    for cfg in CONFIGS:
        clean, = eng80.op_spk_cluster([S], cfg)
        dirty, = _check(eng80, [bad.astype(np.float32)], cfg)
        assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(clean, dirty))


def test_several_streams_in_one_call(eng80):
    mixed = [_cosines(n, seed=s + 1) for s, n in enumerate([5, 0, 70, 1, 131])]
    cfg = dict(threshold=0.3, min_cluster=2)
    alone = [eng80.op_spk_cluster([S], cfg)[0] for S in mixed]
    same = lambda a, b: all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))
    for order in (mixed, mixed[::-1]):
        ref = alone if order is mixed else alone[::-1]
        for _ in range(2):                                         # and again: nothing of a call is left for the next
            got = _check(eng80, order, cfg)
            assert all(same(g, r) for g, r in zip(got, ref))


def test_the_cap(eng80):
    n = 8192                                                       # PF_SPK_MAX_WINDOWS
    S = np.full((n, n), 0.1, np.float32)
    for (i, j), v in {(4000, 8000): 0.95, (3, 4000): 0.9, (3, 8000): 0.9, (10, 8191): 0.8, (0, 1): 0.7, (5000, 5001): 0.6}.items():
        S[i, j] = v
    (labels, k, merges, _), = _check(eng80, [S], dict(min_cluster=1))
    assert k == n - 5 and merges[:6].tolist() == [[4000, 8000], [3, 4000], [10, 8191], [0, 1], [5000, 5001], [-1, -1]]
    assert labels[8000] == labels[4000] == labels[3] == 2 and labels[8191] == labels[10] and labels[-2] == k - 1
    one = np.zeros(1, np.float32)
    out = np.zeros(2, np.int32)
    rc = eng80._lib.pf_op_spk_cluster(eng80._h, one.ctypes.data_as(C.POINTER(C.c_float)), (C.c_int32 * 1)(n + 1), 1, None,
                                      out.ctypes.data_as(C.POINTER(C.c_int32)), out.ctypes.data_as(C.POINTER(C.c_int32)), None, None)
    assert rc == N.PF_ERR_INVALID_ARG


def test_through_the_recogniser(rec_paths, eng80):
    from aliparaformerasr_amd.offline_recognizer import OfflineRecognizer
    paths, cam, _, _ = rec_paths
    audio = [R.two_source_audio(1), V_burst(7, [(100, 400)], 2), np.zeros(16000, np.float32)]
    host = OfflineRecognizer(*paths)                               # never sees the switch
    host.SetSpeakerModel(cam, R.TWO_SOURCE_SPK)
    host.SetVad(VAD_CFG)
    st_h, res_h, census_h = _census(host, audio)
    dev = OfflineRecognizer(*paths)
    dev.SetSpeakerClustering("device")                             # before the model and the VAD: inert until both are there
    dev.SetSpeakerModel(cam, R.TWO_SOURCE_SPK)
    dev.SetVad(VAD_CFG)
    st_d, res_d, census_d = _census(dev, audio)

    def speakers(streams):
        return [(s.SpeakerWindows, s.SegmentSpeakers, np.asarray(s.SpeakerCentroids).tobytes()) for s in streams]

    assert res_d == res_h and _segments(st_d) == _segments(st_h) and speakers(st_d) == speakers(st_h)
    assert st_d[0].SegmentSpeakers == [0, 1, 0, 1]
    # the census: the forward's 15 launches, the affinity, and one prep and one merge launch; every other class as on the host
    assert census_h["spk"] == 16 and census_d["spk"] == 18
    assert {c: v for c, v in census_d.items() if c != "spk"} == {c: v for c, v in census_h.items() if c != "spk"}
    dev.SetSpeakerClustering("host")
    st_b, res_b, census_b = _census(dev, audio)
    assert res_b == res_h and census_b == census_h and speakers(st_b) == speakers(st_h)
    dev.SetSpeakerClustering("device")
    for rec in (dev, host):
        rec.SetSpeakerModel(None)
    (st_off, res_off, census_off), (st_never, res_never, census_never) = _census(dev, audio), _census(host, audio)
    assert res_off == res_never and census_off == census_never and census_off["spk"] == 0
    assert _segments(st_off) == _segments(st_never) and all(s.SegmentSpeakers == [] for s in st_off)
