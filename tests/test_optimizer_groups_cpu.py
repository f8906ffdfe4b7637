"""Parameter groups on the host: GraphormerModel.optimizer_groups (module structure only), the grouped optimizer state dict of
checkpoint.py, and the launcher's flag validation.  No device: FusedAdam is only constructed, never stepped."""
import math
import re
from types import SimpleNamespace

import pytest
import torch

from oracle import cases
from tests.util_model import model_args

ENC = "encoder.graph_encoder."


def _build(shape, **over):
    """"tiny": oracle Tiny A (4-block encoders, 2 of them in one fusion stack).  "launch": the shipped launch's structure — 12-block
    encoders, 8 + 1 blocks in fusion stacks of 2, graph stacks of 2, --freeze_initial_encoders — with small FFNs and vocabulary."""
    from multimodaldiscussiontransformer_amd.models import GraphormerModel
    hp = cases.tiny_hparams("A")
    torch.manual_seed(11)
    if shape == "launch":
        a = model_args(hp, num_fusion_layers=8, num_fusion_stack=2, num_graph_stack=2, freeze_initial_encoders=True, **over)
        a.bert_config = dict(a.bert_config, layers=12, intermediate=64, vocab=100)
        a.vit_config = dict(a.vit_config, layers=12, intermediate=64)
    else:
        a = model_args(hp, **over)
    return GraphormerModel.build_model(a, task=None)


def expected_layer(name, model):
    """(layer id, L) from the parameter's NAME alone, or None outside the pretrained stacks: the test's own reading of the issue's
    rule, independent of encoder_layer_ids()."""
    ge = model.encoder.graph_encoder
    if not name.startswith(ENC):
        return None
    n = name[len(ENC):]
    for model_name, side, cfg in (("text_model", "bert_encoder", ge.bert_config), ("vit_model", "vit_encoder", ge.vit_config)):
        depth = cfg["layers"]
        prefix = len(getattr(ge, model_name).encoder.layer)
        if n.startswith(model_name + ".embeddings."):
            return 0, depth
        m = re.match(model_name + r"\.encoder\.layer\.(\d+)\.", n)
        if m:
            return int(m.group(1)) + 1, depth
        m = re.match(r"fusion_layers\.(\d+)\.fusion_layers\.(\d+)\." + side + r"\.", n)
        if m:
            per = len(ge.fusion_layers[0].fusion_layers)
            return prefix + int(m.group(1)) * per + int(m.group(2)) + 1, depth
    return None


def scale_map(groups):
    return {id(p): (g["lr_scale"], g["weight_decay"]) for g in groups for p in g["params"]}


FLAGS = [dict(), dict(encoder_lr_scale=0.1), dict(encoder_layer_decay=0.5), dict(no_decay_bias_norm=True),
         dict(encoder_lr_scale=0.25, encoder_layer_decay=0.75, no_decay_bias_norm=True), dict(encoder_lr_scale=0.0)]


@pytest.mark.parametrize("shape", ["tiny", "launch"])
def test_optimizer_groups_by_name(shape):
    model = _build(shape)
    named = dict(model.named_parameters())
    trainable = {id(p) for p in model.parameters() if p.requires_grad}
    frozen = {id(p) for p in model.parameters() if not p.requires_grad}
    assert (len(frozen) > 0) == (shape == "launch")
    seen_fusion = seen_prefix = 0
    for kw in FLAGS:
        groups = model.optimizer_groups(weight_decay=0.01, **kw)
        listed = [id(p) for g in groups for p in g["params"]]
        assert len(listed) == len(set(listed)), f"{kw}: a parameter is in two groups"
        assert set(listed) == trainable, f"{kw}: the groups do not hold exactly the trainable parameters"
        assert not set(listed) & frozen
        assert len({(g["lr_scale"], g["weight_decay"]) for g in groups}) == len(groups), "two groups with one record"
        got = scale_map(groups)
        s, d = kw.get("encoder_lr_scale", 1.0), kw.get("encoder_layer_decay", 1.0)
        for name, p in named.items():
            if not p.requires_grad:
                continue
            lay = expected_layer(name, model)
            want = 1.0 if lay is None else s * d ** (lay[1] + 1 - lay[0])
            want_wd = 0.0 if kw.get("no_decay_bias_norm") and p.ndim <= 1 else 0.01
            assert got[id(p)] == (want, want_wd), f"{kw} {name}: {got[id(p)]}, want {(want, want_wd)}"
            if lay is not None:
                seen_fusion += "fusion_layers" in name
                seen_prefix += ".encoder.layer." in name
        if not kw:
            assert len(groups) == 1 and groups[0]["lr_scale"] == 1.0 and groups[0]["weight_decay"] == 0.01
    assert seen_fusion > 0 and (seen_prefix > 0 or shape == "launch")
    # everything the issue lists as scale 1 is there and has scale 1 under the strongest flags
    got = scale_map(model.optimizer_groups(encoder_lr_scale=0.25, encoder_layer_decay=0.5, weight_decay=0.01))
    for frag in ("text_model.pooler.", "vit_model.pooler.", "layers.0.", "graph_node_feature.", "graph_attn_bias.", "bottle_neck.",
                 "bert_projection.", "vit_projection.", "node_classifier.", "masked_lm_pooler.", "lm_head_transform_weight."):
        hit = [n for n, p in named.items() if frag in n and p.requires_grad and expected_layer(n, model) is None]
        assert hit, frag
        assert all(got[id(named[n])][0] == 1.0 for n in hit), frag
    if shape == "tiny":
        assert got[id(named[ENC + "vit_model.layernorm.weight"])][0] == 1.0


def test_prefix_or_fusion_placement_does_not_matter():
    """The same 4-block encoders with 1 + 1 and with 2 + 1 blocks sliced into fusion layers: block i has the same scale."""
    a, b = _build("tiny"), _build("tiny", num_fusion_layers=2)
    ga, gb = a.encoder.graph_encoder, b.encoder.graph_encoder
    assert len(ga.text_model.encoder.layer) == 2 and len(gb.text_model.encoder.layer) == 1
    kw = dict(encoder_lr_scale=0.5, encoder_layer_decay=0.75, weight_decay=0.01)
    sa, sb = scale_map(a.optimizer_groups(**kw)), scale_map(b.optimizer_groups(**kw))

    def blocks(ge, model, side):
        return list(model.encoder.layer) + [getattr(fl, side) for st in ge.fusion_layers for fl in st.fusion_layers]

    for model_name, side in (("text_model", "bert_encoder"), ("vit_model", "vit_encoder")):
        ba, bb = blocks(ga, getattr(ga, model_name), side), blocks(gb, getattr(gb, model_name), side)
        assert len(ba) == len(bb) == 4
        for i, (x, y) in enumerate(zip(ba, bb)):
            want = 0.5 * 0.75 ** (4 - i)
            for p, q in zip(x.parameters(), y.parameters()):
                assert sa[id(p)][0] == sb[id(q)][0] == want, (model_name, i)
    ids = a.encoder_layer_ids()
    assert ids[id(ga.text_model.embeddings.word_embeddings.weight)] == (0, 4)
    assert ids[id(ga.vit_model.embeddings.cls_token)] == ids[id(ga.vit_model.embeddings.position_embeddings)] == (0, 4)
    assert id(ga.vit_model.layernorm.weight) not in ids and id(ga.text_model.pooler.dense.weight) not in ids


# ---------------------------------------------------------------------------------------------------------------- checkpoints
def _opt(model, grouped, **kw):
    from multimodaldiscussiontransformer_amd.optim import FusedAdam
    params = model.optimizer_groups(weight_decay=0.01, **kw) if grouped else [p for p in model.parameters() if p.requires_grad]
    opt = FusedAdam(params, lr=3e-5, weight_decay=0.01)
    return opt


def _mark(opt, model):
    """A recognisable state by POSITION in the trainable list."""
    from multimodaldiscussiontransformer_amd.checkpoint import _trainable
    for i, p in enumerate(_trainable(model)):
        opt.state[id(p)]["m"].fill_(0.001 * (i + 1))
        opt.state[id(p)]["v"].fill_(0.002 * (i + 1))
    opt.step_count = 17


def _marked(opt, model):
    from multimodaldiscussiontransformer_amd.checkpoint import _trainable
    return all(float(opt.state[id(p)]["m"].view(-1)[0]) == pytest.approx(0.001 * (i + 1), rel=1e-6)
               and float(opt.state[id(p)]["v"].view(-1)[0]) == pytest.approx(0.002 * (i + 1), rel=1e-6) for i, p in enumerate(_trainable(model)))


GROUP_KW = dict(encoder_lr_scale=0.5, encoder_layer_decay=0.5, no_decay_bias_norm=True)


def test_ungrouped_state_dict_is_unchanged():
    from multimodaldiscussiontransformer_amd import checkpoint as ck
    model = _build("tiny")
    for opt in (_opt(model, False), _opt(model, True)):          # no groups, and groups that are all (1, global)
        _mark(opt, model)
        osd = ck.optimizer_state_dict(opt, model)
        n = len(ck._trainable(model))
        assert osd["param_groups"] == [{"lr": 3e-5, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0.01, "amsgrad": False,
                                        "params": list(range(n))}]
        assert sorted(osd["state"]) == list(range(n)) and all(set(v) == {"step", "exp_avg", "exp_avg_sq"} for v in osd["state"].values())


def test_grouped_state_dict_round_trip(capsys):
    from multimodaldiscussiontransformer_amd import checkpoint as ck
    model = _build("tiny")
    opt = _opt(model, True, **GROUP_KW)
    _mark(opt, model)
    osd = ck.optimizer_state_dict(opt, model)
    groups = osd["param_groups"]
    n = len(ck._trainable(model))
    assert len(groups) == len(opt.param_groups) > 2
    assert sorted(i for g in groups for i in g["params"]) == list(range(n)), "the ids are those of the one positional numbering"
    firsts = [g["params"][0] for g in groups]
    assert firsts == sorted(firsts), "groups are written in order of first appearance"
    pos = {id(p): i for i, p in enumerate(ck._trainable(model))}
    for g, og in zip(groups, opt.param_groups):
        assert set(g) == {"lr", "lr_scale", "weight_decay", "betas", "eps", "amsgrad", "params"}
        assert g["lr"] == 3e-5 * g["lr_scale"] and (g["lr_scale"], g["weight_decay"]) == (og["lr_scale"], og["weight_decay"])
        assert g["params"] == [pos[id(p)] for p in og["params"]] and g["betas"] == (0.9, 0.999) and g["eps"] == 1e-8
        assert og["lr"] == g["lr"]
    # grouped file -> grouped optimiser of the same partition: silent, positional, hyper-parameters of the running optimiser
    m2 = _build("tiny")
    o2 = _opt(m2, True, **GROUP_KW)
    o2.lr = 1e-3
    ck.load_optimizer_state_dict(o2, m2, osd)
    assert _marked(o2, m2) and o2.step_count == 17 and o2.lr == 1e-3 and o2.weight_decay == 0.01
    assert capsys.readouterr().err == ""
    assert [(g["lr_scale"], g["weight_decay"]) for g in o2.param_groups] == [(g["lr_scale"], g["weight_decay"]) for g in opt.param_groups]


def test_one_group_file_and_grouped_optimiser_both_ways(capsys):
    from multimodaldiscussiontransformer_amd import checkpoint as ck
    model = _build("tiny")
    plain, grouped = _opt(model, False), _opt(model, True, **GROUP_KW)
    _mark(plain, model)
    _mark(grouped, model)
    one_group, many_groups = ck.optimizer_state_dict(plain, model), ck.optimizer_state_dict(grouped, model)
    # a one-group file into a grouped optimiser: the state arrives, the groups stay, the difference is said once
    m2 = _build("tiny")
    o2 = _opt(m2, True, **GROUP_KW)
    before = [(g["lr_scale"], g["weight_decay"], len(g["params"])) for g in o2.param_groups]
    ck.load_optimizer_state_dict(o2, m2, one_group)
    assert _marked(o2, m2) and o2.step_count == 17
    assert before == [(g["lr_scale"], g["weight_decay"], len(g["params"])) for g in o2.param_groups] and o2.lr == 3e-5
    err = capsys.readouterr().err
    assert err.count("parameter groups") == 1 and "keeping the running" in err
    # a grouped file into an optimiser without groups: positional all the same, its own single rate and decay stay
    m3 = _build("tiny")
    o3 = _opt(m3, False)
    o3.lr, o3.weight_decay = 1e-3, 0.02
    ck.load_optimizer_state_dict(o3, m3, many_groups)
    assert _marked(o3, m3) and o3.step_count == 17 and (o3.lr, o3.weight_decay) == (1e-3, 0.02) and not o3.has_groups
    assert capsys.readouterr().err.count("parameter groups") == 1
    # and the file of today into the optimiser of today behaves as it always did: the file's rate and decay are taken
    m4 = _build("tiny")
    o4 = _opt(m4, False)
    o4.lr = 1e-3
    ck.load_optimizer_state_dict(o4, m4, one_group)
    assert _marked(o4, m4) and o4.lr == 3e-5 and capsys.readouterr().err == ""


def test_fused_adam_accepts_groups_on_the_host():
    from multimodaldiscussiontransformer_amd.optim import FusedAdam
    ps = [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2)), torch.nn.Parameter(torch.zeros(5), requires_grad=False)]
    opt = FusedAdam([{"params": ps[:1], "lr_scale": 0.5}, {"params": ps[1:], "weight_decay": 0.0}], lr=1e-3, weight_decay=0.01)
    assert len(opt.params) == 2 and opt.has_groups
    assert [(g["lr"], g["lr_scale"], g["weight_decay"], len(g["params"])) for g in opt.param_groups] == [(5e-4, 0.5, 0.01, 1), (1e-3, 1.0, 0.0, 1)]
    assert not FusedAdam(ps, lr=1e-3).has_groups and len(FusedAdam(ps, lr=1e-3).param_groups) == 1
    for bad, msg in (([{"params": ps[:2]}, {"params": ps[1:]}], "more than one group"), ([{"params": ps, "lr": 1.0}], "unknown keys"),
                     ([{"lr_scale": 1.0}], "no 'params'"), ([{"params": ps, "lr_scale": -1.0}], "finite and >= 0"),
                     ([{"params": ps, "weight_decay": float("inf")}], "finite and >= 0")):
        with pytest.raises(ValueError, match=msg):
            FusedAdam(bad)


# ---------------------------------------------------------------------------------------------------------------- launcher
@pytest.mark.parametrize("flags,msg", [(["--encoder-lr-scale", "-0.1"], "--encoder-lr-scale"), (["--encoder-lr-scale", "nan"], "--encoder-lr-scale"),
                                       (["--encoder-lr-scale", "inf"], "--encoder-lr-scale"), (["--encoder-layer-decay", "0"], "--encoder-layer-decay"),
                                       (["--encoder-layer-decay", "1.5"], "--encoder-layer-decay"), (["--encoder-layer-decay", "nan"], "--encoder-layer-decay"),
                                       (["--encoder-layer-decay", "-0.5"], "--encoder-layer-decay")], ids=lambda f: " ".join(f) if isinstance(f, list) else None)
def test_launcher_refuses_bad_group_flags(flags, msg):
    from multimodaldiscussiontransformer_amd import train
    with pytest.raises(SystemExit, match=msg):
        train.main(["--dataset-name", "synthetic", "--max-update", "1"] + flags)


def test_launcher_knows_the_flags():
    from multimodaldiscussiontransformer_amd import train
    a = train.build_parser().parse_args(["--encoder-lr-scale", "0.1", "--encoder-layer-decay", "0.9", "--no-decay-bias-norm"])
    assert a.encoder_lr_scale == 0.1 and a.encoder_layer_decay == 0.9 and a.no_decay_bias_norm is True
    b = train.build_parser().parse_args([])
    assert b.encoder_lr_scale == 1.0 and b.encoder_layer_decay == 1.0 and b.no_decay_bias_norm is False
    assert math.isfinite(b.encoder_lr_scale)
