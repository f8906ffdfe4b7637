"""bench.py --dump-outputs on the host (bench.dump_outputs): the files a caller compares, their dtypes and size, and a
gradient sample that follows the parameters, not the arena's layout."""
import numpy as np
import pytest
import torch


@pytest.fixture
def bench(monkeypatch):
    monkeypatch.setenv("MDT_BENCH_OFFICIAL", "1")      # what importing bench.py sets: undone after the test
    import bench
    return bench


def _model(reverse_arena: bool):
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(300, 200), torch.nn.Linear(200, 7))
    ps = list(m.parameters())
    arena = torch.zeros(sum(p.numel() + 64 for p in ps))       # padded slots, like the model's gradient arena
    off = 0
    for p in (reversed(ps) if reverse_arena else ps):
        p.main_grad = arena[off:off + p.numel()].view(p.shape)
        off += p.numel() + 64
    g = torch.Generator().manual_seed(1)
    for p in ps:
        p.main_grad.copy_(torch.randn(p.shape, generator=g))
    return m


@pytest.mark.parametrize("sample", [1000, 1 << 22])
def test_dump_outputs_files_and_layout_independence(bench, tmp_path, monkeypatch, sample):
    monkeypatch.setattr(bench, "DUMP_SAMPLE", sample)
    scal, scale = torch.tensor([3.5, 8.0, 5.0, 2.0, 3.0, 4.0]), torch.tensor(0.125)
    for k, rev in enumerate((False, True)):
        bench.dump_outputs(str(tmp_path / str(k)), _model(rev), scal, scale, with_params=True)
    names = {"scalars", "grad_scale", "grad_norms", "grad_sample", "param_norms", "param_sample"}
    a = {n: np.load(tmp_path / "0" / f"{n}.npy") for n in names}
    b = {n: np.load(tmp_path / "1" / f"{n}.npy") for n in names}
    assert {f.name[:-4] for f in (tmp_path / "0").iterdir()} == names
    for n in names:
        assert a[n].dtype in (np.float32, np.float64)
        assert np.array_equal(a[n], b[n]), n
    m = _model(False)
    total = sum(p.numel() for p in m.parameters())
    assert a["grad_sample"].shape == a["param_sample"].shape == (min(sample, total),)
    if sample >= total:             # every element, in named_parameters() order
        assert np.array_equal(a["grad_sample"], torch.cat([p.main_grad.reshape(-1) for p in m.parameters()]).numpy())
    np.testing.assert_allclose(a["grad_norms"], [float(p.main_grad.double().norm()) for p in m.parameters()], rtol=1e-12)
    assert np.array_equal(a["scalars"], scal.double().numpy()) and a["grad_scale"].tolist() == [0.125]
