"""f3: the classification term of the loss on the GPU kernels (csrc/class_loss.hip,
rgbd_amd.point_loss.class_loss) against torch on the CPU in float64:
``F.cross_entropy(x.double(), target, weight=w.double())`` and its autograd gradient, the target
built here from the same matches with plain indexing.

Measures (both bounded by 1e-5, the project's figure for float32 reductions in another order):
  forward   |loss - ref| / max(1, max|x|)
  backward  max|g - ref_g| / (max(w) / W),  W = sum_i w[t_i]
ATen's own float32 path stays at 4.4e-7 / 3.1e-7 in these measures on the same cases.
RGBD_CLASS_LOSS_ERRORS=<file> appends every case's two figures (kernel and switch-off path)."""
import functools
import os

import pytest
import torch
import torch.nn.functional as F

from rgbd_amd import determinism, ops, point_loss

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5

SHAPES = [(1, 1, 2), (2, 100, 49), (8, 100, 49), (7, 13, 65), (5, 100, 64), (33, 100, 134), (2, 37, 257)]
PATTERNS = ["none", "some", "all"]
SCALES = [1.0, 30.0, 1e4]


def _counts(B, Q, pattern):
    if pattern == "none":
        return [0] * B
    if pattern == "all":
        return [Q] * B
    # about 20 % of the rows, image 0 without a match and the last image with all Q matched
    if B == 1:
        return [max(1, round(0.2 * Q))]
    if B == 2:
        return [0, Q]
    other = min(Q, max(1, (round(0.2 * B * Q) - Q) // (B - 2)))
    return [0] + [other] * (B - 2) + [Q]


def _weights(C1):
    w = torch.ones(C1)
    w[-1] = 0.1
    return w


def _lsa(rows, cols):
    """The batched assignment's result built by hand: the concatenated indices, the host counts
    and the per-image views of them."""
    counts = [int(r.numel()) for r in rows]
    ra = torch.cat(rows).to(DEV) if rows else torch.zeros(0, dtype=torch.long, device=DEV)
    ca = torch.cat(cols).to(DEV) if cols else torch.zeros(0, dtype=torch.long, device=DEV)
    out, o = ops.LsaResult(), 0
    for n in counts:
        out.append((ra[o:o + n], ca[o:o + n]))
        o += n
    out.rows_all, out.cols_all, out.counts = ra, ca, tuple(counts)
    return out


@functools.lru_cache(maxsize=None)
def _case(B, Q, C1, pattern, scale, neg_inf=False):
    """CPU inputs and the float64 reference, built once per case and left unchanged."""
    g = torch.Generator().manual_seed(1000 * B + 10 * Q + C1 + PATTERNS.index(pattern))
    x = torch.randn((B, Q, C1), generator=g) * scale
    rows, cols, labels = [], [], []
    for n in _counts(B, Q, pattern):
        T = n + (3 if n else 0)  # more targets than matches: the columns are a subset
        labels.append(torch.randint(0, C1 - 1, (T,), generator=g))
        rows.append(torch.randperm(Q, generator=g)[:n])
        cols.append(torch.randperm(T, generator=g)[:n])
    target = torch.full((B, Q), C1 - 1, dtype=torch.long)
    for b in range(B):
        target[b, rows[b]] = labels[b][cols[b]]
    holes = None
    if neg_inf:
        # -inf on classes that are no row's target
        holes = torch.rand((B, Q, C1), generator=g) < 0.1
        holes.scatter_(2, target[..., None], False)
        x[holes] = float("-inf")
    w = _weights(C1)
    xr = x.double().requires_grad_(True)
    ref = F.cross_entropy(xr.reshape(B * Q, C1), target.reshape(-1), weight=w.double())
    (ref_g,) = torch.autograd.grad(ref, xr)
    return dict(x=x, w=w, rows=rows, cols=cols, labels=labels, target=target, ref=ref.detach(), ref_g=ref_g,
                W=float(w.double()[target].sum()), holes=holes, xmax=float(x[torch.isfinite(x)].abs().max()))


def _measures(c, loss, grad):
    fwd = abs(float(loss.detach().double().cpu()) - float(c["ref"])) / max(1.0, c["xmax"])
    bwd = float((grad.detach().double().cpu() - c["ref_g"]).abs().max()) / (float(c["w"].max()) / c["W"])
    return fwd, bwd


def _aten(x, w, target):
    """The switch-off arithmetic: nn.CrossEntropyLoss over [B, C, Q] in float32 on the GPU."""
    return torch.nn.CrossEntropyLoss(weight=w)(x.transpose(1, 2), target)


def _record(line):
    path = os.environ.get("RGBD_CLASS_LOSS_ERRORS")
    print(line)
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _run(c, dtype=torch.float32):
    x = c["x"].to(DEV, dtype).requires_grad_(True)
    ind = _lsa(c["rows"], c["cols"])
    loss = point_loss.class_loss(x, c["w"].to(DEV), ind, [t.to(DEV) for t in c["labels"]])
    (grad,) = torch.autograd.grad(loss, x)
    return loss, grad


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("B,Q,C1", SHAPES)
def test_loss_and_gradient_against_float64(B, Q, C1, pattern):
    assert C1 <= point_loss.class_loss_max_classes()
    worst = [0.0, 0.0]
    for scale in SCALES:
        c = _case(B, Q, C1, pattern, scale)
        loss, grad = _run(c)
        assert loss.shape == () and loss.dtype == torch.float32 and grad.shape == (B, Q, C1)
        fwd, bwd = _measures(c, loss, grad)
        xa = c["x"].to(DEV).requires_grad_(True)
        la = _aten(xa, c["w"].to(DEV), c["target"].to(DEV))
        afwd, abwd = _measures(c, la, torch.autograd.grad(la, xa)[0])
        _record(f"({B},{Q},{C1}) {pattern:4s} x{scale:g}: kernel fwd {fwd:.3g} bwd {bwd:.3g} | "
                f"ATen fwd {afwd:.3g} bwd {abwd:.3g}")
        worst = [max(worst[0], fwd), max(worst[1], bwd)]
    assert worst[0] <= TOL and worst[1] <= TOL, worst


def test_saved_target_is_the_reference_target():
    c = _case(8, 100, 49, "some", 1.0)
    ind = _lsa(c["rows"], c["cols"])
    lab = point_loss.labels_all([t.to(DEV) for t in c["labels"]], DEV)
    moff = torch.tensor(point_loss._offsets(ind.counts), dtype=torch.int32, device=DEV)
    toff = torch.tensor(point_loss._offsets(t.numel() for t in c["labels"]), dtype=torch.int32, device=DEV)
    _, wsum, _, target = point_loss.class_loss_forward(c["x"].to(DEV), c["w"].to(DEV), ind.rows_all, ind.cols_all,
                                                       moff, toff, lab)
    assert torch.equal(target.cpu().long(), c["target"].reshape(-1))
    assert abs(float(wsum) - c["W"]) <= 1e-5 * c["W"]


def test_minus_inf_on_non_target_classes():
    """-inf logits away from the targets: a finite loss, exactly zero gradient there, no NaN."""
    B, Q, C1 = 2, 100, 49
    c = _case(B, Q, C1, "some", 1.0, neg_inf=True)
    assert int(c["holes"].sum()) > 100
    loss, grad = _run(c)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all())
    assert bool((grad.cpu()[c["holes"]] == 0).all())
    fwd, bwd = _measures(c, loss, grad)
    _record(f"({B},{Q},{C1}) some x1 with -inf: kernel fwd {fwd:.3g} bwd {bwd:.3g}")
    assert fwd <= TOL and bwd <= TOL


@pytest.mark.parametrize("B,Q,C1", [(2, 100, 49), (7, 13, 65), (2, 37, 257), (1, 1, 2)])
def test_bf16_logits_equal_widened_float32(B, Q, C1):
    """bf16 logits go to the kernel as they are: the loss bits of the float32 kernel on the same
    logits widened, and its gradient rounded once to bf16."""
    c = _case(B, Q, C1, "some", 1.0)
    xb = c["x"].to(DEV, torch.bfloat16)
    ind = _lsa(c["rows"], c["cols"])
    labels, w = [t.to(DEV) for t in c["labels"]], c["w"].to(DEV)
    a = xb.clone().requires_grad_(True)
    b = xb.float().requires_grad_(True)
    la, lb = point_loss.class_loss(a, w, ind, labels), point_loss.class_loss(b, w, ind, labels)
    assert la.dtype == torch.float32 and torch.equal(la.view(torch.int32), lb.view(torch.int32))
    (ga,), (gb,) = torch.autograd.grad(la * 3.0, a), torch.autograd.grad(lb * 3.0, b)
    assert ga.dtype == torch.bfloat16 and torch.equal(ga, gb.to(torch.bfloat16))


def _hf_losses():
    from transformers import Mask2FormerConfig
    from transformers.models.mask2former.modeling_mask2former import Mask2FormerLoss
    cfg = Mask2FormerConfig(num_labels=48)
    wd = {"loss_cross_entropy": 2.0, "loss_mask": 5.0, "loss_dice": 5.0}
    ref, hip = Mask2FormerLoss(cfg, weight_dict=wd).to(DEV), Mask2FormerLoss(cfg, weight_dict=wd).to(DEV)
    hip.__class__ = point_loss.HipMask2FormerLoss
    return ref, hip


def _hf_case():
    B, Q, C1, counts = 3, 100, 49, (5, 0, 23)
    g = torch.Generator().manual_seed(77)
    x = torch.randn((B, Q, C1), generator=g).to(DEV)
    labels = [torch.randint(0, C1 - 1, (n,), generator=g).to(DEV) for n in counts]
    ind = _lsa([torch.randperm(Q, generator=g)[:n] for n in counts], [torch.randperm(n, generator=g) for n in counts])
    return x, labels, ind


def _parent_loss_labels(loss, logits, class_labels, indices):
    """HipMask2FormerLoss.loss_labels as it was before the kernel (the HIP_CLASS_LOSS = False arm
    has to stay this).  Its default branch is ATen's 2-d NLL kernel, whose forward adds block sums
    and the weight total with float atomics: two runs of it on the same inputs differ in the last
    bit, so bits are compared in deterministic mode (the 1-d kernel, fixed order) and the default
    branch within 4 float32 spacings."""
    B, Q, _ = logits.shape
    offs = point_loss._offsets(c.shape[0] for c in class_labels)[:-1]
    tco = point_loss.labels_all(class_labels, DEV).index_select(0, loss._target_flat(indices, offs, DEV))
    target = torch.full((B, Q), fill_value=loss.num_labels, dtype=torch.int64, device=DEV)
    b_idx, q_idx = loss._get_predictions_permutation_indices(indices)
    target.view(-1).index_copy_(0, b_idx * Q + q_idx, tco)
    criterion = torch.nn.CrossEntropyLoss(weight=loss.empty_weight)
    if determinism.is_deterministic():
        return criterion(logits.reshape(B * Q, -1), target.view(-1))
    return criterion(logits.transpose(1, 2), target)


def _same_as_parent(hip_loss, x, labels, ind):
    """loss_labels on the torch path against the restated parent path, loss and gradient."""
    for det in (True, False):
        with determinism.deterministic(det):
            xo, xp = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
            o = hip_loss.loss_labels(xo, labels, ind)["loss_cross_entropy"]
            p = _parent_loss_labels(hip_loss, xp, labels, ind)
            go, gp = torch.autograd.grad(o, xo)[0], torch.autograd.grad(p, xp)[0]
        if det:
            assert torch.equal(o.detach().view(torch.int32), p.detach().view(torch.int32)) and torch.equal(go, gp)
        else:
            assert abs(float(o.detach()) - float(p.detach())) <= 4 * 2.0 ** -23 * abs(float(p.detach()))
            assert float((go - gp).abs().max()) <= 4 * 2.0 ** -23 * float(gp.abs().max())


def test_loss_labels_against_the_library(monkeypatch):
    ref_loss, hip_loss = _hf_losses()
    x, labels, ind = _hf_case()
    xr, xh = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    r = ref_loss.loss_labels(xr, labels, ind)["loss_cross_entropy"]
    assert point_loss.HIP_CLASS_LOSS
    calls = []
    real = point_loss.class_loss
    monkeypatch.setattr(point_loss, "class_loss", lambda *a: calls.append(1) or real(*a))
    h = hip_loss.loss_labels(xh, labels, ind)["loss_cross_entropy"]
    assert calls == [1], "loss_labels did not take the kernel"
    (gr,), (gh,) = torch.autograd.grad(r * 2.0, xr), torch.autograd.grad(h * 2.0, xh)
    w = hip_loss.empty_weight
    target = torch.full((3, 100), 48, dtype=torch.long, device=DEV)
    for b, (i, j) in enumerate(ind):
        target[b, i] = labels[b][j]
    W = float(w.double()[target].sum())
    fwd = abs(float(h.detach()) - float(r.detach())) / max(1.0, float(x.abs().max()))
    bwd = float((gh - gr).abs().max()) / 2.0 / (float(w.max()) / W)
    print(f"loss_labels vs transformers: fwd {fwd:.3g} bwd {bwd:.3g}")
    assert fwd <= TOL and bwd <= TOL

    # switch off: the path from before the kernel, bit for bit, and no kernel call
    monkeypatch.setattr(point_loss, "HIP_CLASS_LOSS", False)
    _same_as_parent(hip_loss, x, labels, ind)
    assert calls == [1]


def test_plain_index_pairs_take_the_library_path(monkeypatch):
    ref_loss, hip_loss = _hf_losses()
    x, labels, ind = _hf_case()

    def refuse(*a):
        raise AssertionError("class_loss called for indices that are no LsaResult")
    monkeypatch.setattr(point_loss, "class_loss", refuse)
    plain = [(i.clone(), j.clone()) for i, j in ind]
    xr, xh = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    r = ref_loss.loss_labels(xr, labels, plain)["loss_cross_entropy"]
    h = hip_loss.loss_labels(xh, labels, plain)["loss_cross_entropy"]
    assert abs(float(h.detach()) - float(r.detach())) <= 1e-6 * abs(float(r.detach()))
    assert float((torch.autograd.grad(h, xh)[0] - torch.autograd.grad(r, xr)[0]).abs().max()) <= 1e-8


def test_more_classes_than_the_kernel_holds_take_aten():
    """C1 above the cap: loss_labels routes to the torch path (no error) and matches it."""
    from transformers import Mask2FormerConfig
    from transformers.models.mask2former.modeling_mask2former import Mask2FormerLoss
    cap = point_loss.class_loss_max_classes()
    C1, B, Q, counts = cap + 1, 2, 9, (4, 0)
    wd = {"loss_cross_entropy": 2.0, "loss_mask": 5.0, "loss_dice": 5.0}
    hip_loss = Mask2FormerLoss(Mask2FormerConfig(num_labels=C1 - 1), weight_dict=wd).to(DEV)
    hip_loss.__class__ = point_loss.HipMask2FormerLoss
    g = torch.Generator().manual_seed(5)
    x = torch.randn((B, Q, C1), generator=g).to(DEV)
    labels = [torch.randint(0, C1 - 1, (n,), generator=g).to(DEV) for n in counts]
    ind = _lsa([torch.randperm(Q, generator=g)[:n] for n in counts], [torch.randperm(n, generator=g) for n in counts])
    assert point_loss.HIP_CLASS_LOSS
    _same_as_parent(hip_loss, x, labels, ind)


def test_repeated_calls_give_equal_bits():
    c = _case(33, 100, 134, "some", 30.0)
    runs = [_run(c) for _ in range(3)]
    for loss, grad in runs[1:]:
        assert torch.equal(loss.view(torch.int32), runs[0][0].view(torch.int32))
        assert torch.equal(grad, runs[0][1])


def test_row_statistics_do_not_depend_on_the_batch():
    """Three images processed alone give the per-row (max, log-sum) bits they have inside a batch
    of eight (their rows fall into other workgroups, at other offsets)."""
    B, Q, C1 = 8, 100, 49
    c = _case(B, Q, C1, "all", 30.0)
    w = c["w"].to(DEV)

    def stats(lo, hi):
        ind = _lsa(c["rows"][lo:hi], c["cols"][lo:hi])
        lab = torch.cat(c["labels"][lo:hi]).to(DEV)
        moff = torch.tensor(point_loss._offsets(ind.counts), dtype=torch.int32, device=DEV)
        toff = torch.tensor(point_loss._offsets(t.numel() for t in c["labels"][lo:hi]), dtype=torch.int32, device=DEV)
        x = c["x"][lo:hi].contiguous().to(DEV)
        _, _, st, tg = point_loss.class_loss_forward(x, w, ind.rows_all, ind.cols_all, moff, toff, lab)
        return st, tg
    full, tfull = stats(0, B)
    part, tpart = stats(2, 5)
    assert torch.equal(part.view(torch.int32), full[:, 2 * Q:5 * Q].contiguous().view(torch.int32))
    assert torch.equal(tpart, tfull[2 * Q:5 * Q])


def test_graph_capture_replays_with_new_logits_and_matches():
    B, Q, C1 = 8, 100, 49
    c, c2 = _case(B, Q, C1, "some", 1.0), _case(B, Q, C1, "some", 30.0)
    w = c["w"].to(DEV)
    labels = [t.to(DEV) for t in c["labels"]]
    ind = _lsa(c["rows"], c["cols"])
    x = c["x"].to(DEV).requires_grad_(True)

    def step():
        loss = point_loss.class_loss(x, w, ind, labels)
        return loss, torch.autograd.grad(loss, x)[0]
    step()  # eager warm-up: the workspace and the offset constants exist before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gl, gg = step()
    # new logits and other matches of the same counts, written into the buffers the graph reads
    g = torch.Generator().manual_seed(9)
    new_rows = torch.cat([torch.randperm(Q, generator=g)[:n] for n in ind.counts])
    new_cols = torch.cat([torch.randperm(t.numel(), generator=g)[:n] for t, n in zip(c["labels"], ind.counts)])
    with torch.no_grad():
        x.copy_(c2["x"])
        ind.rows_all.copy_(new_rows)
        ind.cols_all.copy_(new_cols)
    graph.replay()
    torch.cuda.synchronize()
    el, eg = step()
    assert torch.equal(gl.view(torch.int32), el.view(torch.int32)) and torch.equal(gg, eg)
    target = torch.full((B * Q,), C1 - 1, dtype=torch.long)
    o = 0
    for b, n in enumerate(ind.counts):
        target[b * Q + new_rows[o:o + n]] = c["labels"][b][new_cols[o:o + n]]
        o += n
    ref = F.cross_entropy(c2["x"].double().reshape(B * Q, C1), target, weight=c["w"].double())
    assert abs(float(gl) - float(ref)) <= TOL * max(1.0, c2["xmax"])


def test_device_operation_counts():
    """Every device operation the wrapper issues — kernels, memsets, copies — is a node of a
    captured graph: at most 3 for the forward (target build included), 1 for the backward, in
    one chain."""
    from rgbd_amd.graph_guard import graph_width
    B, Q, C1 = 8, 100, 49
    c = _case(B, Q, C1, "some", 1.0)
    w, labels, ind = c["w"].to(DEV), [t.to(DEV) for t in c["labels"]], _lsa(c["rows"], c["cols"])
    seed = torch.ones((), device=DEV)
    for dtype in (torch.float32, torch.bfloat16):
        x = c["x"].to(DEV, dtype).requires_grad_(True)

        def fwd():
            return point_loss.class_loss(x, w, ind, labels)

        def both():
            return torch.autograd.grad(fwd(), x, grad_outputs=seed)
        both()  # warm-up
        torch.cuda.synchronize()
        nodes = []
        for fn in (fwd, both):
            graph = torch.cuda.CUDAGraph(keep_graph=True)
            with torch.cuda.graph(graph):
                out = fn()
            width, n = graph_width(graph.raw_cuda_graph())
            assert width == 1
            nodes.append(n)
            del out, graph
        print(f"{dtype}: forward {nodes[0]} device operations, forward + backward {nodes[1]}")
        assert 1 <= nodes[0] <= 3 and nodes[1] - nodes[0] == 1, nodes


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,Q,C1", [(7, 13, 65), (2, 100, 49)])
def test_guard_bands(B, Q, C1, dtype):
    """One forward + backward with every output, saved tensor and workspace between guard bands,
    and the inputs too: no guard byte changes, and the results are those of plain buffers."""
    from checkers import guard
    c = _case(B, Q, C1, "some", 1.0)
    want_loss, want_grad = _run(c, dtype)
    with guard.guarded_allocations() as sw:
        x = sw.place(c["x"].to(DEV, dtype), "logits").requires_grad_(True)
        lsa = _lsa(c["rows"], c["cols"])
        ind = _lsa(c["rows"], c["cols"])
        ind.rows_all, ind.cols_all = sw.place(lsa.rows_all, "rows_all"), sw.place(lsa.cols_all, "cols_all")
        labels = [sw.place(t.to(DEV), "labels") if t.numel() else t.to(DEV) for t in c["labels"]]
        loss = point_loss.class_loss(x, sw.place(c["w"].to(DEV), "weight"), ind, labels)
        (grad,) = torch.autograd.grad(loss, x)
        assert sw.check_all() >= 9 and sw.passed_through == 0
        assert len(sw.workspaces()) == 1
    assert torch.equal(loss.view(torch.int32), want_loss.view(torch.int32)) and torch.equal(grad, want_grad)
