"""bench.py --dump-outputs: what ``bench.snapshot_outputs`` reads from a ``Trainer`` built with
``keep_outputs`` after a captured (HIP-graph) step, at batch 8 -- every parameter, the momentum buffer
and every layer's forward output, float32, the outputs sampled at the same indices in every run, and
the kept outputs are the graph's own tensors (a replay rewrites them).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_snapshot_outputs_of_graph_step(cuda_device, monkeypatch, tmp_path):
    import bench
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 1000)
    layers, xs, gs = bench.build(cuda_device, 8, seed=1234, data_seed=1235)
    tr = bench.Trainer(layers, 1, keep_outputs=True)
    tr.step(xs, gs)  # the initialising step
    tr.flat.zero_()
    tr.capture(xs, gs)
    tr.step_graph(xs, gs)
    torch.cuda.synchronize()
    first = bench.snapshot_outputs(tr)
    assert bench.snapshot_outputs(tr).keys() == first.keys()
    for k in tr.kept:
        k.zero_()
    tr.step_graph(xs, gs)
    torch.cuda.synchronize()
    second = bench.snapshot_outputs(tr)

    names = {f"{spec[0]}.{pn}" for spec, m in zip(bench.RESNET20, layers) for pn, _ in m.named_parameters()}
    names |= {f"{spec[0]}.out" for spec in bench.RESNET20} | {"momentum"}
    assert set(second) == names
    assert sum(a.nbytes for a in second.values()) <= 64 * 2 ** 20
    for i, (spec, y) in enumerate(zip(bench.RESNET20, tr.kept)):
        name = spec[0]
        a = second[name + ".out"]
        assert a.dtype == np.float32 and a.shape == (min(1000, y.numel()),)
        assert np.isfinite(a).all() and np.abs(a).max() > 0, name  # the replay wrote the kept tensor again
        # the sample: the layer's own seeded indices of the flat output
        idx = np.sort(np.random.default_rng(i).integers(0, y.numel(), 1000))
        assert np.array_equal(a, y.reshape(-1).cpu().numpy()[idx]), name
    for k, a in second.items():
        assert a.dtype == np.float32 and np.isfinite(a).all(), k
    assert not np.array_equal(first["conv1.weight"], second["conv1.weight"])  # a later step's parameters
    assert second["momentum"].shape == (tr.opt.buf.numel(),)

    bench.dump_outputs(second, str(tmp_path / "out"))
    for k, a in second.items():
        assert np.array_equal(np.load(tmp_path / "out" / (k + ".npy")), a)
