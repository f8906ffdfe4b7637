"""--store-ema on the host: the averaged weights travel in a FairSeq checkpoint as extra_state["ema"] (an fp32 state dict under
the model's keys, q/k/v split as the weights are), come back bit for bit — whatever is reset —, a file without the key seeds the
average from the restored weights, a run without the flag neither writes nor needs the key, and the launcher refuses the EMA
flags without --store-ema before it touches a device."""
from types import SimpleNamespace

import pytest
import torch

from tests.test_checkpoint_cpu import _tiny


def _opt(model, **kw):
    from multimodaldiscussiontransformer_amd.optim import FusedAdam
    return FusedAdam([p for p in model.parameters() if p.requires_grad], lr=3e-5, weight_decay=0.01, **kw)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _args():
    return SimpleNamespace(task="node_prediction", arch="multi_graphormer_base", criterion="node_cross_entropy", seed=1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_ema_round_trips_through_a_checkpoint(tmp_path, dtype):
    from multimodaldiscussiontransformer_amd import checkpoint as ck
    _, model = _tiny(dtype=dtype)
    opt = _opt(model, ema_decay=0.9)
    assert opt.ema_arena.dtype == torch.float32
    for p in opt.params:                                       # seeded from the master (bf16) or the fp32 parameter
        src = opt.state[id(p)].get("master", p.detach())
        assert torch.equal(_bits(opt.state[id(p)]["ema"]), _bits(src.float()))
    gen = torch.Generator().manual_seed(3)
    opt.ema_arena.copy_(torch.randn(opt.ema_arena.shape, generator=gen))          # fp32 values no bf16 holds
    sd = opt.ema_state_dict(model)
    msd = model.state_dict()
    assert set(sd) <= set(msd) and all(v.dtype == torch.float32 and tuple(v.shape) == tuple(msd[k].shape) for k, v in sd.items())
    assert any(".query." in k or ".q_proj." in k for k in sd), "q/k/v are stored as the three parts"
    path = str(tmp_path / "with_ema.pt")
    ck.save_checkpoint(path, model, _args(), optimizer=opt, num_updates=5, extra_state={"ema": sd})
    raw = torch.load(path, map_location="cpu", weights_only=False)
    assert list(raw["extra_state"]["ema"]) == list(sd) and "train_iterator" in raw["extra_state"]
    for kw in (dict(), dict(reset_optimizer=True, reset_meters=True, reset_lr_scheduler=True, reset_dataloader=True)):
        _, m2 = _tiny(dtype=dtype)
        o2 = _opt(m2, ema_decay=0.9)
        info = ck.load_checkpoint(path, m2, optimizer=o2, **kw)
        assert info["ema"] is not None, "the average is model state: no reset drops it"
        o2.load_ema_state_dict(m2, info["ema"])
        for p, q in zip(opt.params, o2.params):             # (slot by slot: the arena pads every slot to 16 bytes)
            assert torch.equal(_bits(o2.state[id(q)]["ema"]), _bits(opt.state[id(p)]["ema"]))
    # a run without the flag ignores the key
    _, m3 = _tiny(dtype=dtype)
    o3 = _opt(m3)
    info = ck.load_checkpoint(path, m3, optimizer=o3)
    assert o3.ema_arena is None and info["num_updates"] == 5
    # a missing or a foreign key raises, as a strict model load does; so does another shape
    short = dict(sd)
    k0 = next(iter(short))
    v0 = short.pop(k0)
    with pytest.raises(RuntimeError, match="missing keys"):
        opt.load_ema_state_dict(model, short)
    with pytest.raises(RuntimeError, match="unexpected keys"):
        opt.load_ema_state_dict(model, dict(sd, **{"encoder.nothing.weight": v0}))
    with pytest.raises(ValueError, match="shape"):
        opt.load_ema_state_dict(model, dict(sd, **{k0: torch.zeros(v0.numel() + 1)}))


def test_file_without_the_key_seeds_from_the_restored_weights(tmp_path):
    from multimodaldiscussiontransformer_amd import checkpoint as ck
    _, model = _tiny(dtype=torch.bfloat16)
    plain = _opt(model)
    for p in plain.params:
        plain.state[id(p)]["master"].mul_(1.0 + 2.0 ** -12)                         # masters that are no bf16 numbers
    path = str(tmp_path / "plain.pt")
    ck.save_checkpoint(path, model, _args(), optimizer=plain, num_updates=2, extra_state={"val_loss": None})
    raw = torch.load(path, map_location="cpu", weights_only=False)
    assert "ema" not in raw["extra_state"]
    torch.manual_seed(99)
    _, m2 = _tiny(dtype=torch.bfloat16)
    o2 = _opt(m2, ema_decay=0.9999, ema_start_update=3)
    info = ck.load_checkpoint(path, m2, optimizer=o2)
    assert info["ema"] is None
    o2.seed_ema_from_weights()
    for p, q in zip(plain.params, o2.params):
        assert torch.equal(_bits(o2.state[id(q)]["ema"]), _bits(plain.state[id(p)]["master"]))


def test_optimiser_refuses_what_makes_no_sense():
    _, model = _tiny()
    with pytest.raises(ValueError):
        _opt(model, ema_decay=1.5)
    with pytest.raises(ValueError):
        _opt(model, ema_decay=0.9, ema_update_freq=0)
    plain = _opt(model)
    for call in (lambda: plain.ema_state_dict(model), lambda: plain.load_ema_state_dict(model, {}), plain.seed_ema_from_weights):
        with pytest.raises(RuntimeError, match="ema_decay"):
            call()


@pytest.mark.parametrize("flags", [["--ema-decay", "0.9"], ["--ema-start-update", "10"], ["--ema-update-freq", "2"], ["--ema-fp32"],
                                   ["--validate-with-ema"]], ids=lambda f: f[0])
def test_launcher_refuses_ema_flags_without_store_ema(flags):
    from multimodaldiscussiontransformer_amd import train
    with pytest.raises(SystemExit, match="without --store-ema"):
        train.main(["--dataset-name", "synthetic", "--max-update", "1"] + flags)


def test_launcher_knows_the_flags():
    from multimodaldiscussiontransformer_amd import train
    a = train.build_parser().parse_args(["--store-ema", "--ema-decay", "0.99", "--ema-start-update", "7", "--ema-update-freq", "3", "--ema-fp32",
                                         "--validate-with-ema"])
    assert a.store_ema and a.ema_decay == 0.99 and a.ema_start_update == 7 and a.ema_update_freq == 3 and a.ema_fp32 and a.validate_with_ema
    b = train.build_parser().parse_args([])
    assert not b.store_ema and b.ema_decay is None and b.validate_with_ema is None
    with pytest.raises(SystemExit, match=r"\[0, 1\]"):
        train.main(["--dataset-name", "synthetic", "--store-ema", "--ema-decay", "1.5"])
