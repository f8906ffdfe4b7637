"""Parameter groups through the launcher on the synthetic task, Tiny model, --deterministic, bf16 (fp32 masters): the flags at
their defaults change nothing, --encoder-layer-decay / --no-decay-bias-norm give every parameter the update of its own group, and a
grouped run with the weight average and --clip-norm on saves, restores and continues bit for bit in one Adam launch per table."""
import pytest
import torch

import tests.adam_groups_reference as A
import tests.loss_optim_reference as R
from tests.test_grad_clip_gpu import _launcher_argv

pytestmark = pytest.mark.gpu

BASE = ["--deterministic", "--bf16", "--disable-validation"]


def _bits(t):
    return t.detach().contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu()


def _same_tree(a, b, path=""):
    """Two checkpoint trees are equal: tensors by bits, everything else by ==."""
    if torch.is_tensor(a):
        assert torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape, path
        assert torch.equal(_bits(a), _bits(b)) if a.dtype in (torch.float32, torch.bfloat16) else torch.equal(a, b), path
    elif isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), f"{path}: keys {sorted(set(map(str, a)) ^ set(map(str, b)))}"
        for k in a:
            _same_tree(a[k], b[k], f"{path}/{k}")
    elif isinstance(a, (list, tuple)):
        assert type(a) is type(b) and len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same_tree(x, y, f"{path}[{i}]")
    else:
        assert a == b, f"{path}: {a!r} != {b!r}"


def _final():
    from multimodaldiscussiontransformer_amd import train
    opt = train.main.last_run["optimizer"]
    return ([_bits(p.data) for p in opt.params], [_bits(opt.state[id(p)]["master"]) for p in opt.params],
            [_bits(opt.state[id(p)]["m"]) for p in opt.params], [_bits(opt.state[id(p)]["v"]) for p in opt.params],
            [_bits(opt.state[id(p)]["ema"]) for p in opt.params] if opt.ema_arena is not None else [])


def test_default_flags_are_the_run_without_them(tmp_path, capsys):
    from multimodaldiscussiontransformer_amd import train
    h0 = train.main(_launcher_argv(BASE + ["--max-update", "3", "--save-dir", str(tmp_path / "a")]))
    assert not train.main.last_run["optimizer"].has_groups
    h1 = train.main(_launcher_argv(BASE + ["--max-update", "3", "--save-dir", str(tmp_path / "b"), "--encoder-lr-scale", "1",
                                           "--encoder-layer-decay", "1.0"]))
    assert not train.main.last_run["optimizer"].has_groups
    assert "optimizer_groups" not in capsys.readouterr().out
    strip = lambda h: [{k: v for k, v in m.items() if k != "wall"} for m in h]          # noqa: E731
    assert strip(h0) == strip(h1) and len(h0) == 3 and all("lr_min" not in m for m in h1)
    a = torch.load(tmp_path / "a" / "checkpoint_last.pt", weights_only=False)
    b = torch.load(tmp_path / "b" / "checkpoint_last.pt", weights_only=False)
    for st in (a, b):
        st["extra_state"].pop("previous_training_time")
        st["cfg"]["model"].pop("save_dir")                      # the two runs write to two directories, and the cfg says where
    _same_tree(a, b)
    assert not {"encoder_lr_scale", "encoder_layer_decay", "no_decay_bias_norm"} & set(a["cfg"]["model"])
    assert len(a["last_optimizer_state"]["param_groups"]) == 1 and "lr_scale" not in a["last_optimizer_state"]["param_groups"][0]


def test_every_parameter_takes_the_update_of_its_own_group(monkeypatch, capsys):
    """--encoder-layer-decay 0.5 --no-decay-bias-norm, 3 updates: at every update each parameter's master, m and v are within the
    reference's bound of the fp64 update of ITS group (lr_t, step_size_t, wd_t) from the stored state and gradient."""
    from multimodaldiscussiontransformer_amd import optim, train
    real = optim.FusedAdam.step
    seen = []

    def step(self, lr=None, grad_scale=None, num_updates=None):
        before = [(self.state[id(p)]["master"].detach().cpu().view(-1), self.state[id(p)]["m"].cpu().view(-1), self.state[id(p)]["v"].cpu().view(-1),
                   p.main_grad.detach().cpu().view(-1).clone()) for p in self.params]
        real(self, lr=lr, grad_scale=grad_scale, num_updates=num_updates)
        torch.cuda.synchronize()
        guard = dict(scale=float(self.grad_scale_used), skip=0, skipped=0, step_size=0.0)
        hyp = dict(lr=lr, beta1=self.betas[0], beta2=self.betas[1], eps=self.eps, wd=self.weight_decay)
        for p, (p0, m0, v0, g) in zip(self.params, before):
            ref = A.reference_tensor(p0, g, m0, v0, hyp, self.step_count, self.hyper_of(p), None, guard)
            st = self.state[id(p)]
            what = f"update {self.step_count} {tuple(p.shape)} {self.hyper_of(p)}"
            R.check("train groups p", st["master"].cpu().view(-1), ref["p"], what)
            R.check("train groups m", st["m"].cpu().view(-1), ref["m"], what)
            R.check("train groups v", st["v"].cpu().view(-1), ref["v"], what)
            assert torch.equal(_bits(p.data), _bits(st["master"].to(torch.bfloat16))), what
        seen.append(self.step_count)

    monkeypatch.setattr(optim.FusedAdam, "step", step)
    hist = train.main(_launcher_argv(BASE + ["--max-update", "3", "--no-save", "--weight-decay", "0.05", "--encoder-layer-decay", "0.5",
                                             "--no-decay-bias-norm"]))
    assert seen == [1, 2, 3] and len(hist) == 3
    opt, model = train.main.last_run["optimizer"], train.main.last_run["model"]
    # 2-block encoders: embeddings 0.5^3, block 0 0.5^2, block 1 0.5; everything else 1; no decay on vectors
    want = {id(p): (g["lr_scale"], g["weight_decay"]) for g in model.optimizer_groups(encoder_layer_decay=0.5, no_decay_bias_norm=True, weight_decay=0.05)
            for p in g["params"]}
    assert all(opt.hyper_of(p) == want[id(p)] for p in opt.params)
    assert {opt.hyper_of(p)[0] for p in opt.params} == {1.0, 0.5, 0.25, 0.125}
    assert all(opt.hyper_of(p)[1] == (0.0 if p.ndim <= 1 else 0.05) for p in opt.params)
    assert all(m["lr_min"] == m["lr"] * 0.125 for m in hist)
    out = capsys.readouterr().out
    assert out.count('"optimizer_groups"') == 1


ALL = ["--deterministic", "--bf16", "--store-ema", "--ema-decay", "0.9", "--validate-interval-updates", "2", "--validate-with-ema", "--clip-norm", "0.05",
       "--encoder-lr-scale", "0.5", "--encoder-layer-decay", "0.75", "--no-decay-bias-norm"]


def test_grouped_run_saves_restores_and_continues_bit_for_bit(tmp_path, monkeypatch):
    """All three flags with the weight average and --clip-norm on: trains, validates, saves, restores in one process; every Adam
    launch is the ONE grouped launch of its dtype table; the resumed run ends on the uninterrupted run's bits."""
    from multimodaldiscussiontransformer_amd import optim, train

    class Spy:
        def __init__(self, real):
            self._real, self.names = real, []

        def __getattr__(self, name):
            self.names.append(name)
            return getattr(self._real, name)

    spy = Spy(optim.lib)
    monkeypatch.setattr(optim, "lib", spy)
    hist = train.main(_launcher_argv(ALL + ["--max-update", "4", "--save-dir", str(tmp_path), "--save-interval-updates", "2"]))
    opt = train.main.last_run["optimizer"]
    adam = [n for n in spy.names if n.startswith("mdt_adam_step")]
    assert adam == ["mdt_adam_step_multi_groups"] * (4 * len(opt._tables())), adam
    assert [h["num_updates"] for h in hist] == [1, 2, 3, 4] and any(h["clip"] > 0 for h in hist)
    assert [v["num_updates"] for v in train.main.valid_history] == [2, 4] and all(v["weights"] == "ema" for v in train.main.valid_history)
    whole = _final()
    ck = tmp_path / "checkpoint_1_2.pt"
    st = torch.load(ck, weights_only=False)
    groups = st["last_optimizer_state"]["param_groups"]
    assert len(groups) == len(opt.param_groups) > 2 and all(g["lr"] == opt.lr * g["lr_scale"] for g in groups)
    assert st["cfg"]["model"]["encoder_layer_decay"] == 0.75 and st["cfg"]["model"]["no_decay_bias_norm"] is True
    resumed = train.main(_launcher_argv(ALL + ["--max-update", "4", "--restore-file", str(ck), "--no-save"]))
    assert [h["num_updates"] for h in resumed] == [3, 4]
    assert [(h["loss"], h["gnorm"], h["lr_min"]) for h in resumed] == [(h["loss"], h["gnorm"], h["lr_min"]) for h in hist[2:]]
    for x, y in zip(_final(), whole):
        assert len(x) == len(y) and all(torch.equal(a, b) for a, b in zip(x, y)), "the resumed run differs from the uninterrupted one"
