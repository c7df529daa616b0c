"""hipGraph replay of the train step (tg_hip.graph.GraphedTrainStep) is bit-identical to the eager step: losses, generated
batch, every weight, BatchNorm buffer and Adam moment after several steps -- at the reference's own CPU-runnable case
(256x256, batch 1: BASELINE configs[0]) and at its shipped batch size 2 (train.py:77)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tg_hip import lib
    lib.load()
    return torch.device("cuda:0")


def _build(dev):
    from mvp_gan.src.models import Discriminator, PConvUNet
    from mvp_gan.src.utils.losses import InpaintingLoss
    torch.manual_seed(0)
    G, D = PConvUNet(), Discriminator()
    crit = InpaintingLoss(0.1, 0.1, device=torch.device("cpu"))
    G, D, crit = G.to(dev), D.to(dev), crit.to(dev)
    return G, D, crit, torch.optim.Adam(G.parameters(), lr=2e-4), torch.optim.Adam(D.parameters(), lr=2e-4)


@pytest.mark.parametrize("b,size", [(1, 256), (2, 128)])
def test_graphed_step_is_bit_identical_to_eager(dev, b, size):
    from mvp_gan.src.train import train_step
    from oracle import terragan_oracle as Orc
    from tg_hip.graph import GraphedTrainStep
    nsteps = 6
    data = [tuple(t.to(dev) for t in Orc.synth_batch(b, size, 50 + s)) for s in range(nsteps)]
    keys = ("g_total", "g_loss", "g_adv", "d_loss", "real_loss", "fake_loss")
    runs = {}
    for mode in ("eager", "graph"):
        G, D, crit, oG, oD = _build(dev)
        step = GraphedTrainStep(G, D, crit, oG, oD, warmup=2) if mode == "graph" else None
        losses, gens = [], []
        for real, mask in data:
            out = step(real, mask) if step is not None else train_step(G, D, crit, oG, oD, real, mask)
            losses.append(tuple(float(out[k]) for k in keys))          # read before the next replay overwrites the statics
            gens.append(out["gen"].detach().clone())
        if step is not None:
            assert step.replays == nsteps - 2
            step.flush()
        torch.cuda.synchronize()
        runs[mode] = (losses, gens, {k: v.detach().clone() for m in (G, D) for k, v in m.state_dict().items()},
                      [(int(st["step"]), st["exp_avg"].clone(), st["exp_avg_sq"].clone()) for o in (oG, oD) for st in o.state.values()])
    assert runs["eager"][0] == runs["graph"][0], (runs["eager"][0], runs["graph"][0])
    for a, c in zip(runs["eager"][1], runs["graph"][1]):
        assert torch.equal(a, c)
    for k, v in runs["eager"][2].items():
        assert torch.equal(v, runs["graph"][2][k]), k
    for (s1, m1, v1), (s2, m2, v2) in zip(runs["eager"][3], runs["graph"][3]):
        assert s1 == s2 == nsteps and torch.equal(m1, m2) and torch.equal(v1, v2)


def test_graphed_step_rejects_another_batch_shape(dev):
    from oracle import terragan_oracle as Orc
    from tg_hip.graph import GraphedTrainStep
    G, D, crit, oG, oD = _build(dev)
    step = GraphedTrainStep(G, D, crit, oG, oD, warmup=1)
    real, mask = (t.to(dev) for t in Orc.synth_batch(2, 128, 3))
    for _ in range(3):
        step(real, mask)
    real2, mask2 = (t.to(dev) for t in Orc.synth_batch(3, 128, 3))
    with pytest.raises(ValueError):
        step(real2, mask2)


def test_eager_ops_between_replays_see_the_replayed_weights(dev):
    """A replay rewrites G / D weights on the device; the host-side prepared-weight cache must not serve transforms of older
    weights to eager work done between replays -- the reference validates between train steps (train.py:278-301: G.eval()
    forward at the validation batch's size, D in train mode).  Compared with the same sequence run with the cache off."""
    from oracle import terragan_oracle as Orc
    from tg_hip import ops as O
    from tg_hip.graph import GraphedTrainStep
    from mvp_gan.src.train import validation_step
    data = [tuple(t.to(dev) for t in Orc.synth_batch(2, 128, 70 + s)) for s in range(5)]
    vdata = [tuple(t.to(dev) for t in Orc.synth_batch(3, 96, 90 + s)) for s in range(2)]          # another size AND batch
    runs = {}
    for cache in (True, False):
        O.WPREP_CACHE = cache
        try:
            G, D, crit, oG, oD = _build(dev)
            step = GraphedTrainStep(G, D, crit, oG, oD, warmup=1) if cache else None
            from mvp_gan.src.train import train_step
            rec = []
            for i, (real, mask) in enumerate(data):
                out = step(real, mask) if step is not None else train_step(G, D, crit, oG, oD, real, mask)
                rec.append(float(out["g_total"]))
                if i >= 1:                                   # from the first replay on: eager validation in between
                    G.eval()
                    for vr, vm in vdata:
                        gt, dl = validation_step(G, D, crit, vr, vm)
                        rec += [float(gt), float(dl)]
                    with torch.no_grad():
                        rec.append(float(D(data[0][0]).sum()))         # D forward at the TRAIN size: the non-batchable entries
                    G.train()
            torch.cuda.synchronize()
            if step is not None:
                assert step.replays == len(data) - 1
            runs[cache] = (rec, {k: v.detach().clone() for m in (G, D) for k, v in m.state_dict().items()})
        finally:
            O.WPREP_CACHE = True
    assert runs[True][0] == runs[False][0], (runs[True][0], runs[False][0])
    for k, v in runs[False][1].items():
        assert torch.equal(v, runs[True][1][k]), k


# ---- host-side changes between two replays of a live trainer ----------------------------------------------------------------
# A change made by the host between step i and step i + 1 must reach the captured step exactly as it reaches the eager one: the
# reference is the identical sequence on train_step, compared bit for bit (losses, generated batch, every state_dict tensor,
# Adam moments and step counts after flush()).  B = 2 at 128x128 (the shipped batch size, and the smallest configuration here in
# which batchable and non-batchable prepared entries both occur), warmup = 1, six steps, the change after step 3: two replays on
# either side.  The unchanged eager run is computed once and shared: each test asserts that its change moved the losses.
KEYS = ("g_total", "g_loss", "g_adv", "d_loss", "real_loss", "fake_loss")
NSTEPS, CHANGE_AFTER = 6, 3
_shared = {}


def _data(dev):
    from oracle import terragan_oracle as Orc
    if "data" not in _shared:
        _shared["data"] = [tuple(t.to(dev) for t in Orc.synth_batch(2, 128, 50 + s)) for s in range(NSTEPS)]
    return _shared["data"]


def _sequence(dev, graphed, hook=None, nsteps=NSTEPS):
    """Six steps, hook(i, ctx) after step i (1-based).  -> dict(losses, gens, sd, adam, step, replays_at: replays before step i)."""
    from mvp_gan.src.train import train_step
    from tg_hip.graph import GraphedTrainStep
    G, D, crit, oG, oD = _build(dev)
    step = GraphedTrainStep(G, D, crit, oG, oD, warmup=1) if graphed else None
    ctx = {"G": G, "D": D, "oG": oG, "oD": oD, "step": step, "dev": dev, "data": _data(dev), "notes": []}
    ctx["sd0"] = [{k: v.detach().clone() for k, v in m.state_dict().items()} for m in (G, D)]
    losses, gens, replays_at = [], [], []
    for i, (real, mask) in enumerate(_data(dev)[:nsteps], start=1):
        replays_at.append(step.replays if step is not None else 0)
        out = step(real, mask) if step is not None else train_step(G, D, crit, oG, oD, real, mask)
        losses.append(tuple(float(out[k]) for k in KEYS))          # read before the next replay overwrites the statics
        gens.append(out["gen"].detach().clone())
        if hook is not None:
            hook(i, ctx)
    replays_at.append(step.replays if step is not None else 0)
    if step is not None:
        step.flush()
    torch.cuda.synchronize()
    return {"losses": losses, "gens": gens, "notes": ctx["notes"], "step": step, "replays_at": replays_at,
            "sd": {f"{n}.{k}": v.detach().clone() for n, m in (("G", G), ("D", D)) for k, v in m.state_dict().items()},
            "adam": [(int(st["step"]), st["exp_avg"].clone(), st["exp_avg_sq"].clone()) for o in (oG, oD) for st in o.state.values()]}


def _plain(dev):
    if "plain" not in _shared:
        _shared["plain"] = _sequence(dev, False)
    return _shared["plain"]


def _assert_same(eager, graph):
    assert eager["losses"] == graph["losses"], (eager["losses"], graph["losses"])
    assert eager["notes"] == graph["notes"], (eager["notes"], graph["notes"])
    for i, (a, c) in enumerate(zip(eager["gens"], graph["gens"])):
        assert torch.equal(a, c), f"gen of step {i + 1}"
    assert eager["sd"].keys() == graph["sd"].keys()
    for k, v in eager["sd"].items():
        assert torch.equal(v, graph["sd"][k]), k
    assert len(eager["adam"]) == len(graph["adam"]) > 0
    for (s1, m1, v1), (s2, m2, v2) in zip(eager["adam"], graph["adam"]):
        assert s1 == s2 and torch.equal(m1, m2) and torch.equal(v1, v2), (s1, s2)


def _assert_not_vacuous(graph, first_change=CHANGE_AFTER, last_change=CHANGE_AFTER):
    step, at = graph["step"], graph["replays_at"]
    assert step.wprep_keys, "the captured step refreshes no prepared weights: nothing here could go stale"
    assert at[first_change] >= 2, f"{at[first_change]} replays before the change"
    assert at[-1] - at[last_change] >= 2, f"{at[-1] - at[last_change]} replays after the change"


def _assert_mattered(dev, eager, after=CHANGE_AFTER):
    plain = _plain(dev)
    assert plain["losses"][:after] == eager["losses"][:after]
    for i in range(after, NSTEPS):
        assert plain["losses"][i] != eager["losses"][i], f"the change left the losses of step {i + 1} as they were"


def _both(dev, hook):
    eager, graph = _sequence(dev, False, hook), _sequence(dev, True, hook)
    _assert_not_vacuous(graph)
    return eager, graph


def test_checkpoint_weights_restored_between_replays(dev):
    """a. G.load_state_dict / D.load_state_dict of the step-0 weights after step 3 (in-place copies: torch bumps the versions);
    the optimisers keep their moments.  The replays that follow must run forward AND dgrad on the restored weights."""
    def hook(i, ctx):
        if i == CHANGE_AFTER:
            ctx["G"].load_state_dict(ctx["sd0"][0])
            ctx["D"].load_state_dict(ctx["sd0"][1])
    eager, graph = _both(dev, hook)
    _assert_mattered(dev, eager)
    _assert_same(eager, graph)


def test_data_write_and_weights_updated_between_replays(dev):
    """b. The documented out-of-band protocol: every 4-D weight of G scaled through `.data`, then ops.weights_updated()."""
    from tg_hip import ops as O

    def hook(i, ctx):
        if i == CHANGE_AFTER:
            for p in ctx["G"].parameters():
                if p.dim() == 4:
                    p.data.mul_(0.5)
            O.weights_updated(ctx["G"].parameters())
    eager, graph = _both(dev, hook)
    _assert_mattered(dev, eager)
    _assert_same(eager, graph)


def test_weights_swapped_in_used_eagerly_and_swapped_back_between_replays(dev):
    """c. EMA-style evaluation: other weights copied into D, an eager D forward at the TRAIN geometry (which re-prepares into the
    very buffers the graph reads), the training weights copied back, and no eager op after that.  The eager reference of this
    sequence computes the losses of the unchanged run (the swap leaves no trace in an eager trainer's weights: asserted), so `the
    change mattered` is asserted on the swap itself: D's output with the foreign weights differs from its output with the
    training weights on the same batch."""
    def hook(i, ctx):
        if i == CHANGE_AFTER:
            D, x = ctx["D"], ctx["data"][0][0]
            with torch.no_grad():
                own = float(D(x).sum())
                mine = {k: v.detach().clone() for k, v in D.state_dict().items()}
                D.load_state_dict(ctx["sd0"][1])
                foreign = float(D(x).sum())
                D.load_state_dict(mine)                     # (buffers too: the BatchNorm running statistics of the foreign forward)
            ctx["notes"] += [own, foreign]
    eager, graph = _both(dev, hook)
    assert eager["losses"] == _plain(dev)["losses"]
    own, foreign = eager["notes"]
    assert own != foreign, "D gave the same value with the foreign weights: the swap is not exercised"
    _assert_same(eager, graph)


def test_learning_rate_changed_between_replays(dev):
    """d. A scheduler: param_groups[*]['lr'] of both optimisers set after step 3 and again after step 4."""
    lrs = {3: 1e-3, 4: 5e-5}

    def hook(i, ctx):
        if i in lrs:
            for opt in (ctx["oG"], ctx["oD"]):
                for group in opt.param_groups:
                    group["lr"] = lrs[i]
    eager, graph = _sequence(dev, False, hook), _sequence(dev, True, hook)
    _assert_not_vacuous(graph, 3, 4)
    _assert_mattered(dev, eager, after=4)                  # (the rate of step 4 shows in the losses of step 5)
    plain = _plain(dev)
    assert any(not torch.equal(v, plain["sd"][k]) for k, v in eager["sd"].items())
    _assert_same(eager, graph)


def test_changed_betas_or_eps_between_replays_raise(dev):
    """e. betas and eps are arguments of the captured Adam launches: the call after such a change raises and replays nothing."""
    from tg_hip.graph import GraphedTrainStep
    G, D, crit, oG, oD = _build(dev)
    step = GraphedTrainStep(G, D, crit, oG, oD, warmup=1)
    data = _data(dev)
    for real, mask in data[:3]:
        step(real, mask)
    assert step.wprep_keys and step.replays == 2
    oD.param_groups[0]["betas"] = (0.5, 0.999)
    with pytest.raises(ValueError, match="betas"):
        step(*data[3])
    assert step.replays == 2
    oD.param_groups[0]["betas"] = (0.9, 0.999)
    oG.param_groups[0]["eps"] = 1e-6
    with pytest.raises(ValueError, match="eps"):
        step(*data[3])
    assert step.replays == 2
    torch.cuda.synchronize()


def test_optimizer_state_restored_between_replays_recaptures(dev):
    """f. optimizer.load_state_dict() of a snapshot taken after step 1, after step 3: the moments are other tensors now, the
    pointers in the captured Adam tables are gone.  The trainer drops its graph, runs `warmup` steps eagerly and captures again."""
    import copy

    def hook(i, ctx):
        if i == 1:
            ctx["snap"] = [copy.deepcopy(o.state_dict()) for o in (ctx["oG"], ctx["oD"])]
        if i == CHANGE_AFTER:
            before = [st["exp_avg"].data_ptr() for st in ctx["oG"].state.values()]
            ctx["oG"].load_state_dict(ctx["snap"][0])
            ctx["oD"].load_state_dict(ctx["snap"][1])
            assert before != [st["exp_avg"].data_ptr() for st in ctx["oG"].state.values()], "the restore is expected to replace the moments"
    eager, graph = _sequence(dev, False, hook), _sequence(dev, True, hook)
    step, at = graph["step"], graph["replays_at"]
    assert step.wprep_keys and at[CHANGE_AFTER] >= 2 and at[-1] - at[CHANGE_AFTER] >= 2, at
    assert step.captures == 2
    assert eager["adam"][0][0] == NSTEPS - 2                # the restored count (1) + the three steps after it
    _assert_mattered(dev, eager, after=CHANGE_AFTER + 1)     # (restored moments show in the weights of step 4, the losses of step 5)
    _assert_same(eager, graph)


def test_unchanged_replay_makes_no_launch_of_its_own(dev, monkeypatch, tmp_path):
    """The checks in front of a replay are host-side comparisons: an unchanged replay calls into the library for its Adam scalars
    (host arithmetic + ONE tg_write_floats launch) and for nothing else, and records no conv launch; a replay after a reported
    weight write adds exactly one tg_conv_wprep_run."""
    import collections
    from tg_hip import lib as L
    from tg_hip import ops as O
    from tg_hip.graph import GraphedTrainStep
    G, D, crit, oG, oD = _build(dev)
    step = GraphedTrainStep(G, D, crit, oG, oD, warmup=1)
    data = _data(dev)
    for real, mask in data[:3]:
        step(real, mask)
    assert step.wprep_keys and step.replays == 2
    torch.cuda.synchronize()
    lib, calls = L.load(), collections.Counter()
    for name in L.SIGNATURES:
        def counted(*a, _fn=getattr(lib, name), _name=name):
            calls[_name] += 1
            return _fn(*a)
        monkeypatch.setattr(lib, name, counted)
    for kind in (0, 1, 2, 3):
        lib.tg_prof_summary(kind, None, None, None, None)
    lib.tg_prof_enable(1)
    calls.clear()
    try:
        step(*data[3])
        unchanged = dict(calls)
        torch.cuda.synchronize()
    finally:
        lib.tg_prof_enable(0)
    path = str(tmp_path / "launches.csv")
    assert lib.tg_prof_dump(path.encode()) == 0
    rows = open(path).read().strip().splitlines()[1:]
    for kind in (0, 1, 2, 3):
        lib.tg_prof_summary(kind, None, None, None, None)
    print("library calls of an unchanged replay:", unchanged, "recorded conv launches:", len(rows))
    assert rows == []
    assert unchanged == {"tg_adam_scalars": len(step.arena.slots), "tg_write_floats": 1}, unchanged
    for p in G.parameters():
        if p.dim() == 4:
            p.data.mul_(0.5)
    O.weights_updated(G.parameters())
    calls.clear()
    step(*data[4])
    changed = dict(calls)
    torch.cuda.synchronize()
    print("library calls of a replay after a reported weight write:", changed)
    assert changed == {"tg_adam_scalars": len(step.arena.slots), "tg_write_floats": 1, "tg_conv_wprep_run": 1}, changed


def test_capture_finds_the_tables_of_its_warmup_step_in_a_full_table_cache(dev, monkeypatch):
    """The descriptor tables of the batched weight preparation are cached, a bounded number of them.  The capture needs the two
    tables its warm-up step made (it cannot build one: a host-to-device copy), so making the discriminator's must not evict the
    generator's -- with the cache full of other models' tables when the trainer starts."""
    from tg_hip import ops as O
    from tg_hip.graph import GraphedTrainStep
    monkeypatch.setattr(O, "_wprep_tables", {("another model", i): None for i in range(O.WPREP_TABLES_MAX)})
    G, D, crit, oG, oD = _build(dev)
    step = GraphedTrainStep(G, D, crit, oG, oD, warmup=1)
    losses = []
    for real, mask in _data(dev)[:3]:
        out = step(real, mask)
        losses.append(tuple(float(out[k]) for k in KEYS))
    torch.cuda.synchronize()
    assert step.wprep_keys and step.replays == 2 and step.captures == 1
    assert len(O._wprep_tables) <= O.WPREP_TABLES_MAX
    assert losses == _plain(dev)["losses"][:3]
