"""CPU: the host statement the device clustering is compared with (pf_host_spk_cluster_trace: the trace only records) and the
`cluster=` key of the CLI's -spk option."""
import numpy as np
import pytest

import spk_ref as R
from aliparaformerasr_amd import engine as E
from aliparaformerasr_amd import examples as X


@pytest.mark.parametrize("cfg", [{}, dict(threshold=0.25, min_cluster=2), dict(num_speakers=3)])
@pytest.mark.parametrize("n", [0, 1, 2, 40])
def test_trace_records_the_walk_and_changes_nothing(n, cfg):
    rng = np.random.default_rng(n)
    S = R.affinity(rng.standard_normal((3, 8))[rng.integers(0, 3, n)] + 0.4 * rng.standard_normal((n, 8))).astype(np.float32).reshape(n, n)
    labels, k, merges, heights = E.host_spk_cluster_trace(S, cfg)
    plain_labels, plain_k = E.host_spk_cluster(S, cfg)
    assert labels.tolist() == plain_labels.tolist() == R.cluster(S, **cfg)[0].tolist() and k == plain_k
    used = (merges >= 0).all(axis=1)
    m = int(used.sum())
    assert used[:m].all() and (merges[m:] == -1).all() and (heights[m:] == 0).all()
    assert (merges[:m, 0] < merges[:m, 1]).all() and len(set(merges[:m, 1].tolist())) == m       # a cluster dies once
    if m:
        assert heights[0] == np.triu(S.astype(np.float64), 1)[np.triu_indices(n, 1)].max()       # the first merge: the largest cosine
    if "num_speakers" in cfg:
        assert m == max(n - 3, 0)
    else:
        assert (heights[:m] >= np.float32(cfg.get("threshold", 0.5))).all()


def test_cli_cluster_key():
    assert X.split_spk_cluster("threshold=0.3,cluster=device,min_cluster=2") == ("threshold=0.3,min_cluster=2", "device")
    assert X.split_spk_cluster("cluster=host") == ("", "host") and X.split_spk_cluster("win=100") == ("win=100", None)
    with pytest.raises(ValueError):
        X.split_spk_cluster("cluster=gpu")
    base = ["-type", "offline", "-vad", "-files", "a.wav"]
    want = {"file": "cam.pfw", "cfg": {"threshold": 0.4}, "cluster": "device"}
    assert X.parse_args(["-spk", "cam.pfw,cluster=device", "threshold=0.4"] + base)["spk"] == want
    assert X.parse_args(["-spk", "cam.pfw", "threshold=0.4,cluster=device"] + base)["spk"] == want
    with pytest.raises(ValueError):
        X.parse_spk_option("cluster=device")                       # not a pf_spk_config key: the CLI takes it apart first
