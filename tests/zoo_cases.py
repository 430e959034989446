"""What every per-model test does with a fixture of tests/golden/ (conftest.Golden), written once: build the model
from the fixture, compare a forward, a training trajectory, a captured-graph replay and a drop-in run of the
reference's own class with what the reference recorded.  A plain module: no fixtures, hooks or plugins; a test hands
its `monkeypatch` / `tmp_path` in as ordinary arguments.

Stated tolerances (BASELINE.json north_star: logits within 1e-4 fp32 of the reference forward): logits 1e-4,
predictions atol 2e-5, losses 1e-4 per step, trained weights through conftest.assert_weights_close, integer and
boolean tensors exactly."""
import contextlib

import numpy as np
import torch

from conftest import assert_weights_close

LOGIT_TOL = 1e-4
OMIT = object()      # as a keyword's value in build_from_golden: leave that keyword of the common block out


def tb(b):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in b.items()}


def allow_cpu_optimizer(monkeypatch):
    """The product optimizer refuses CPU parameters; lift exactly that check, so that the CPU emulations can train."""
    from fuxictr_amd import optim
    orig = optim._NativeOptimizer.__init__

    def init(self, params, lr, model=None, **kw):
        self._require_cuda = False
        orig(self, params, lr, model=model, **kw)
    monkeypatch.setattr(optim._NativeOptimizer, "__init__", init)


def build_from_golden(model_cls, g, tmp_path, gpu=-1, **model_kw):
    """`model_cls` with the fixture's hyper-parameters and initial weights.  `model_kw` maps the family's own `meta`
    entries to its keywords and may replace any keyword of the common block (OMIT removes one)."""
    from fuxictr_amd.features import FeatureMap
    m = g.meta
    fmap = FeatureMap(g.spec["dataset_id"], str(tmp_path))
    fmap.load_dict(g.spec, {"embedding_dim": m["embedding_dim"]})
    kw = dict(model_id=m["name"], gpu=gpu, embedding_dim=m["embedding_dim"], learning_rate=m["lr"],
              optimizer=m["optimizer"], loss="binary_crossentropy", task="binary_classification",
              metrics=["logloss", "AUC"], verbose=0, model_root=str(tmp_path),
              embedding_regularizer=m.get("emb_reg", 0), net_regularizer=m.get("net_reg", 0), sparse_update="exact")
    kw.update(model_kw)
    model = model_cls(fmap, **{k: v for k, v in kw.items() if v is not OMIT})
    sd = {k: torch.from_numpy(v) for k, v in g.state0.items()}
    got = model.state_dict()
    assert sorted(got.keys()) == sorted(sd.keys())                        # the reference's checkpoint keys
    for k, v in sd.items():
        assert tuple(got[k].shape) == tuple(v.shape) and got[k].dtype == v.dtype, k
    result = model.load_state_dict(sd, strict=True)
    assert not result.missing_keys and not result.unexpected_keys
    model._max_gradient_norm = m["max_norm"]
    return model


def _forward(model, g):
    model.eval()                                   # (on the device: flushes pending zero-gradient steps)
    with torch.no_grad():
        return model.forward(tb(g.batches[-1]))["y_pred"]


def check_forward(model, g, which):
    """The eval forward of the last batch against `logit<which>` / `pred<which>`, "0" before and "1" after the
    recorded steps -> (max |logit - reference|, the predictions), for a test that holds them tighter."""
    p = _forward(model, g)
    err = np.abs(p._fx_logit.reshape(-1).cpu().numpy() - g.expect["logit" + which]).max()
    print(g.meta["name"], "max |logit%s - reference| %.3e" % (which, err))
    assert err <= LOGIT_TOL, err
    pred = p.reshape(-1).cpu().numpy()
    np.testing.assert_allclose(pred, g.expect["pred" + which], atol=2e-5)
    return err, pred


def _check_weights(model, g):
    sd = model.state_dict()
    for k, ref in g.state1.items():
        got = sd[k].cpu().numpy()
        if ref.dtype.kind in "ib":
            assert np.array_equal(got, ref), k
        else:
            assert_weights_close(got, ref, g.meta["lr"], g.meta["steps"], k)


def _train(model, g, per_step):
    model.train()
    losses = []
    for i in range(g.meta["steps"]):
        with per_step(i):
            losses.append(float(model.train_step(tb(g.batches[i])).item()))
    print(g.meta["name"], "max |loss - reference| %.3e" % np.abs(np.asarray(losses) - g.expect["loss"]).max())
    np.testing.assert_allclose(losses, g.expect["loss"], rtol=0, atol=1e-4)


def check_trajectory(model, g, per_step=None):
    """The recorded steps: the losses, then the forward and every weight of `state1`.  `per_step(i)` is a context
    manager entered around step i (the host tests' launch counters)."""
    _train(model, g, per_step or (lambda i: contextlib.nullcontext()))
    check_forward(model, g, "1")
    _check_weights(model, g)
    if next(model.parameters()).is_cuda:
        model.optimizer.check_errors()


def check_graph_replay(build, g, steps=9):
    """`hip_graph: true` replays the captured step: same kernels, same order -> same bits as `build(hip_graph=False)`;
    the capture really happened (`_graph_state`), it did not fall back to eager."""
    eager, graph = build(hip_graph=False), build(hip_graph=True)
    eager.train()
    graph.train()
    n = len(g.batches)
    for i in range(steps):                   # eager warm-ups + probe + replays
        b = tb(g.batches[i % n])
        le = float(eager.train_step(b).item())
        lg = float(graph.train_step(b).item())
        assert le == lg, (i, le, lg)
    assert graph._graph_state is not None
    eager.eval()
    graph.eval()
    se, sg = eager.state_dict(), graph.state_dict()
    for k in se:
        assert torch.equal(se[k], sg[k]), k
    graph.optimizer.check_errors()


def check_dropin(model_cls, g, tmp_path, layer_types, calls=None, forward_calls=None, final_calls=None, **model_kw):
    """The reference's own `model_cls`, constructed after patch.install(), reproduces the fixture it produced on the
    stock layers.  `layer_types` lists (attribute, class) the patch must have put in; `calls` is the host file's
    launch counter (where it has one), which has to read `forward_calls` after the first forward and `final_calls`
    after the steps and the second forward."""
    calls = {} if calls is None else calls
    model = build_from_golden(model_cls, g, tmp_path, sparse_update=OMIT, **model_kw)
    for attr, cls in layer_types:
        assert type(getattr(model, attr)) is cls, attr
    for k in calls:
        calls[k] = 0
    pred0 = _forward(model, g).reshape(-1).numpy()          # (the reference's forward keeps no logit)
    np.testing.assert_allclose(pred0, g.expect["pred0"], atol=2e-5)
    assert calls == (forward_calls or {})
    for k in calls:
        calls[k] = 0
    _train(model, g, lambda i: contextlib.nullcontext())
    np.testing.assert_allclose(_forward(model, g).reshape(-1).numpy(), g.expect["pred1"], atol=2e-5)
    _check_weights(model, g)
    assert calls == (final_calls or {})
