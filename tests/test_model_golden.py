"""GPU: the full product model (HIP path) on the golden step-2 scenario generated from the
reference: logits of all three forwards, both losses, every gradient, BN side effects."""
import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from oracle import rap_oracle as O
from tests import helpers as Hh
from tests.test_hip_parity import close

pytestmark = pytest.mark.gpu


def _build(golden, dev):
    import mdil_ss_amd  # noqa: F401
    from mdil_ss_amd.models.erfnet_RA_parallel import Net
    from mdil_ss_amd import ops
    ops.invalidate_packs()        # fresh parameter storage: forget packed images of older models
    teacher_sd, student_sd = Hh.golden_scenario(golden)
    student = Net([20, 20], 2, 1)
    student.load_state_dict(student_sd)
    teacher = Net([20], 1, 0)
    teacher.load_state_dict(teacher_sd)
    student.to(dev)
    teacher.to(dev)
    for p in teacher.parameters():
        p.requires_grad = False
    for n, p in student.named_parameters():
        p.requires_grad = O.step2_trainable("module." + n, 1)
    return student, teacher


@pytest.mark.parametrize("sink", [False, True])
def test_step2_iteration_against_reference_golden(golden, sink):
    """sink=True re-homes the parameters into engine.FlatAdam's flat buffers, so weight / bias /
    BN-affine gradients are accumulated by the kernels straight into the flat gradient buffer
    (the path bench.py and the trainer use); sink=False returns them through autograd."""
    dev = torch.device("cuda:0")
    from mdil_ss_amd import ops
    from mdil_ss_amd.engine import FlatAdam
    student, teacher = _build(golden, dev)
    names = [n for n, _ in student.named_parameters()]
    assert ["module." + n for n in names] == list(golden["param_names"])
    if sink:
        named = [("module." + n, p) for n, p in student.named_parameters()]
        FlatAdam([{"params": [p for n, p in named if O.is_shared(n)], "lr": 5e-6},
                  {"params": [p for n, p in named if O.is_ds_curr(n, 1)]}])
    m_new, m_old = Hh.golden_masks(golden, 0)
    queue = [m_new, m_old]
    student.mask_provider = lambda n: queue.pop(0)
    images = torch.from_numpy(golden["it0_images"]).to(dev)
    labels = torch.from_numpy(golden["it0_labels"]).to(dev)
    weight = torch.tensor(fx.WEIGHT_BDD, device=dev)
    student.train()
    teacher.eval()
    ops.GATE_LOG = []          # the ReLU gates the HIP forwards apply (new-task graph first), read only
    out_new = student(images, 1)
    out_prev = student(images, 0)
    hip_gates, ops.GATE_LOG = ops.GATE_LOG, None
    with torch.no_grad():
        out_teacher = teacher(images, 0)
    close(out_teacher, torch.from_numpy(golden["it0_logits_prev_model"]), rtol=5e-4, atol=5e-5,
          what="teacher (eval) logits")
    close(out_new, torch.from_numpy(golden["it0_logits_new"]), rtol=5e-4, atol=5e-5,
          what="student new-task logits")
    close(out_prev, torch.from_numpy(golden["it0_logits_prev_task"]), rtol=5e-4, atol=5e-5,
          what="student old-task logits")
    ce = ops.cross_entropy2d(out_new, labels[:, 0], weight)
    kld = ops.kld_prob(out_prev, out_teacher)
    total = ce + 0.1 * kld
    np.testing.assert_allclose([ce.item(), kld.item(), total.item()], golden["it0_losses"], rtol=2e-5)
    total.backward()
    ref = golden["it0_grad_digest"]
    params = dict(student.named_parameters())
    got = Hh.digest_rows([params[n].grad for n in names])
    assert np.array_equal(np.isnan(got[:, 0]), np.isnan(ref[:, 0])), "frozen params must have grad None"
    noise = np.array([Hh.zero_grad_bias(n) for n in names])
    ok = ~np.isnan(ref[:, 0]) & ~noise
    # ---- every gradient against the REFERENCE's numbers at ONE fixed tolerance.
    # The fp32 forward agrees with the reference to ~1e-5, and in this tiny scenario (N = 2, 32x64: 64..1024
    # pixels per layer) a handful of the 925,696 ReLU pre-activations lie closer to zero than that: the HIP
    # path takes the other branch there (measured: 1-2 gates, tools/diag_flips.py; same x -> bit-for-bit the
    # same gates, tools/diag_block2.py).  A step function has no small error: one flipped gate in a 256-pixel
    # layer moves every upstream gradient by ~1 %.  Rounds 1-5 absorbed that in a 4 % norm bound (and in a
    # tolerance that depended on WHERE the flip fell).  Now the flips are measured and their effect is
    # MODELLED: the oracle (pinned to the reference on exactly this scenario, tests/test_oracle_golden.py)
    # differentiates once with its own gates -- that IS the golden run -- and once with the gates the HIP
    # forward applied; the difference of the two is what the k flipped gates do to each gradient, and
    #       reference golden  +  (oracle on the HIP gates  -  oracle on its own gates)
    # is what the reference would have computed on those gates.  Every tensor must agree with that at the
    # tolerance of the gate-forced tests (1e-3 relative / 2e-4 of the tensor's largest element), and the
    # number of flips is bounded.
    teacher_sd_c, student_sd_c = Hh.golden_scenario(golden)
    images_c, labels_c = torch.from_numpy(golden["it0_images"]), torch.from_numpy(golden["it0_labels"])
    weight_c = torch.tensor(fx.WEIGHT_BDD)
    assert len(hip_gates) == 2 * 73, len(hip_gates)

    def oracle_grads(gates_new, gates_old, record=None):
        S = {k: v.clone() for k, v in student_sd_c.items()}
        for n in names:
            S[n].requires_grad_(O.step2_trainable("module." + n, 1))
        act = O._act
        try:
            if record is not None:
                O._act = lambda x, gates: (record.append(x.detach() > 0), act(x, gates))[1]
            O.step2_iteration(S, {k: v.clone() for k, v in teacher_sd_c.items()}, images_c, labels_c, weight_c, 1,
                              0.1, m_new, m_old, gates_new, gates_old)
        finally:
            O._act = act
        return {n: S[n].grad for n in names}

    own_gates = []
    g_own = oracle_grads(None, None, record=own_gates)      # new-task forward, old-task forward, frozen model
    assert len(own_gates) >= 2 * 73
    flips_new = [int((h.cpu() != o).sum()) for h, o in zip(hip_gates[:73], own_gates[:73])]
    flips_old = [int((h.cpu() != o).sum()) for h, o in zip(hip_gates[73:], own_gates[73:2 * 73])]
    n_gates = sum(o.numel() for o in own_gates[:2 * 73])
    print(f"relu gates that differ from the oracle's (= the reference's): new-task graph {sum(flips_new)}, "
          f"old-task graph {sum(flips_old)} of {n_gates}")
    assert sum(flips_new) + sum(flips_old) <= 16, (flips_new, flips_old)
    g_hipgates = oracle_grads([g.cpu() for g in hip_gates[:73]], [g.cpu() for g in hip_gates[73:]])
    # the oracle on its own gates IS the golden run (norms; the CPU suite pins it element-wise)
    own_rows = Hh.digest_rows([g_own[n] for n in names])
    np.testing.assert_allclose(own_rows[ok, 2], ref[ok, 2], rtol=1e-4, atol=1e-7)
    worst = ("", 0.0)
    lin = [0] + list(range(3, 67))                 # digest entries that are linear in the tensor: sum + 64 samples
    for i, n in enumerate(names):
        if not ok[i]:
            continue
        delta = (g_hipgates[n] - g_own[n]).detach()
        d_rows = Hh.digest_rows([delta])[0]
        scale = float(g_own[n].abs().max())
        want = ref[i, lin] + d_rows[lin]
        tol = 1e-3 * np.abs(want) + 2e-4 * scale * np.where(np.arange(len(lin)) == 0, g_own[n].numel() ** 0.5, 1.0)
        bad = np.abs(got[i, lin] - want) > tol
        bad[0] &= g_own[n].numel() <= 4096                               # (sums of large tensors cancel: samples only)
        assert not bad.any(), (n, int(bad.sum()), got[i, lin][bad][:4], want[bad][:4], scale)
        # norms: HIP against the oracle on the SAME gates (the reference's norm on other gates is not comparable)
        l2_o = float(g_hipgates[n].norm())
        assert abs(got[i, 2] - l2_o) <= 1e-3 * l2_o + 1e-7, (n, got[i, 2], l2_o)
        key = f"it0_grad_{n}"
        if key in golden.files:                    # 202 tensors of <= 4,096 elements + three large ones
            wantt = torch.from_numpy(golden[key]) + delta
            close(params[n].grad, wantt, rtol=1e-3, atol=2e-4, what=f"grad {n} vs reference golden on the HIP gates")
            rel = float((params[n].grad.detach().cpu() - wantt).norm() / (wantt.norm() + 1e-30))
            if rel > worst[1]:
                worst = (n, rel)
    print(f"gradients vs the reference golden (flipped gates modelled by the oracle): {int(ok.sum())} tensors, "
          f"worst per-tensor rel-L2 over the {sum(1 for n in names if 'it0_grad_' + n in golden.files)} stored in full: "
          f"{worst[1]:.2e} ({worst[0]})")
    assert worst[1] <= 5e-3, worst
    sd = student.state_dict()
    for k, v in sd.items():
        if O.is_buffer(k):
            close(v.float(), torch.from_numpy(golden[f"it0_buf_{k}"]).float(), rtol=5e-4, atol=1e-4,
                  what=f"buffer {k}")


def test_eval_forward_against_reference_golden(golden):
    """The golden's eval-mode logits of both heads were taken by the reference AFTER its two training
    iterations (tools/gen_golden.py: epoch-2 learning rates, Adam from zero moments, the recorded batches
    and dropout masks).  The HIP path repeats exactly that -- two iterations of the shipped Step2Engine (the
    second one on the three-stream schedule), then the folded-BN eval forward -- and its logits are compared
    with the reference's.  (Adam's first updates are lr * sign(g): elements whose gradient is rounding noise
    move by +-lr with a noise-determined sign in ANY two fp32 implementations -- by construction they do
    not move the loss to first order; the oracle reproduces these logits to 1e-6, the bound here is what
    the HIP path measures with margin.)"""
    dev = torch.device("cuda:0")
    from mdil_ss_amd import train_new_task_step2 as T
    from mdil_ss_amd.engine import Step2Engine
    student, teacher = _build(golden, dev)
    T.current_task = 1
    weight = torch.tensor(fx.WEIGHT_BDD, device=dev)
    eng = Step2Engine(student, teacher, weight, current_task=1, lambdac=0.1, is_shared=T.is_shared,
                      is_ds_curr=T.is_DS_curr)
    eng.optimizer.set_epoch(2, 150)
    np.testing.assert_allclose([g["lr"] for g in eng.optimizer.param_groups], golden["lr_values"][1], rtol=1e-12)
    for it in range(2):
        m_new, m_old = Hh.golden_masks(golden, it)
        q = [m_new, m_old]
        student.mask_provider = lambda n: q.pop(0)
        _, ce, kld = eng.iteration(torch.from_numpy(golden[f"it{it}_images"]).to(dev),
                                   torch.from_numpy(golden[f"it{it}_labels"]).to(dev))
        np.testing.assert_allclose([float(ce), float(kld)], golden[f"it{it}_losses"][:2],
                                   rtol=2e-5 if it == 0 else 2e-3)
    assert eng.multi_stream
    student.mask_provider = None
    student.eval()
    images = torch.from_numpy(golden["it0_images"]).to(dev)
    with torch.no_grad():
        for task in (1, 0):
            y = student(images, task).float().cpu()
            r = torch.from_numpy(golden[f"eval_logits_task{task}"])
            assert tuple(y.shape) == tuple(r.shape) == (2, 20, 32, 64)
            rel = float((y - r).norm() / r.norm())
            agree = float((y.argmax(1) == r.argmax(1)).float().mean())
            print(f"eval logits of head {task} after two training iterations vs the reference golden: rel-L2 {rel:.2e}, "
                  f"max |d| {float((y - r).abs().max()):.2e} of {float(r.abs().max()):.2e}, argmax agreement {agree * 100:.3f} %")
            # head 1 is two sign-like Adam steps (lr 5e-4) away from its random init: its logits are 0.2 in size and
            # most pixels are near-ties between classes (measured: rel-L2 4.7e-3, argmax 99.4 %); head 0 and the
            # shared encoder (lr 5e-6) barely move
            lim = (1e-2, 0.985) if task == 1 else (2e-3, 0.998)
            assert rel <= lim[0] and agree >= lim[1], (task, rel, agree)


@pytest.mark.parametrize("async_wgrad", [False, True])
def test_three_stream_schedule_matches_single_stream(golden, async_wgrad, monkeypatch):
    """engine.Step2Engine: the 3-stream lock-step schedule (two gradient sinks, one backward over
    both graphs) must give the same losses and the same flat gradient as the plain single-stream
    iteration on identical inputs and dropout masks -- in the shipped configuration (block-level
    C ABI, block-boundary BN fusion, fused head) and with the side-stream weight-gradient
    experiment (per-launch host path: the block-boundary fusion is off there, so it is switched off
    in the single-stream run too -- like is compared with like)."""
    dev = torch.device("cuda:0")
    from mdil_ss_amd import ops
    if async_wgrad:
        monkeypatch.setattr(ops, "BN_TAIL", False)
    from mdil_ss_amd import train_new_task_step2 as T
    from mdil_ss_amd.engine import Step2Engine
    T.current_task = 1
    images = torch.from_numpy(golden["it0_images"]).to(dev)
    labels = torch.from_numpy(golden["it0_labels"]).to(dev)
    weight = torch.tensor(fx.WEIGHT_BDD, device=dev)
    results = []
    for streams in (False, True):
        student, teacher = _build(golden, dev)
        eng = Step2Engine(student, teacher, weight, current_task=1, lambdac=0.1,
                          is_shared=T.is_shared, is_ds_curr=T.is_DS_curr, streams=streams,
                          async_wgrad=streams and async_wgrad)
        m_new, m_old = Hh.golden_masks(golden, 0)
        q = [m_new, m_old, m_new, m_old]
        student.mask_provider = lambda n: q.pop(0)
        eng.optimizer.step = lambda grad_scale=1.0: None        # keep the gradients for inspection
        # iteration 1 always runs on one stream (it creates the packed weight images); iteration 2
        # is the one compared: it uses the 3-stream schedule when streams=True
        eng.iteration(images, labels)
        total, ce, kld = eng.iteration(images, labels)
        assert bool(getattr(eng, "multi_stream", False)) == streams
        torch.cuda.synchronize()
        results.append((float(ce), float(kld), eng.optimizer.flat_grad.clone()))
        ops.ASYNC_WGRAD = False
    (ce0, kld0, g0), (ce1, kld1, g1) = results
    assert ce0 == pytest.approx(ce1, rel=1e-6) and kld0 == pytest.approx(kld1, rel=1e-6)
    np.testing.assert_allclose([ce0, kld0], golden["it0_losses"][:2], rtol=2e-5)
    # same kernels, same inputs; only the order in which the two graphs' shared-encoder gradients
    # are added differs (g_ce + g_kd vs g_kd + g_ce is exact; partial sums differ at fp32 ulp level)
    close(g1, g0, rtol=1e-5, atol=1e-6, what="flat gradient, 3-stream vs single-stream")


def test_staggered_schedule_is_bit_identical_to_lock_step(golden):
    """engine.Step2Engine (round 4): the staggered three-stream schedule -- the old-domain graph starts k
    plan steps behind the new-domain graph, each graph's backward follows its own loss, optionally with
    the frozen model's forward for the next batch pipelined behind the new-domain backward -- runs the
    same launches in the same per-stream order as the lock-step schedule with ONE backward over both
    graphs: losses, BatchNorm buffers and parameters after three optimizer steps must be bit-identical
    for every stagger and with / without the pipelined frozen model."""
    dev = torch.device("cuda:0")
    from mdil_ss_amd import train_new_task_step2 as T
    from mdil_ss_amd.engine import Step2Engine
    T.current_task = 1
    images = torch.from_numpy(golden["it0_images"]).to(dev)
    labels = torch.from_numpy(golden["it0_labels"]).to(dev)
    weight = torch.tensor(fx.WEIGHT_BDD, device=dev)
    m_new, m_old = Hh.golden_masks(golden, 0)

    def run(stagger, pipelined):
        student, teacher = _build(golden, dev)
        eng = Step2Engine(student, teacher, weight, current_task=1, lambdac=0.1,
                          is_shared=T.is_shared, is_ds_curr=T.is_DS_curr, streams=True)
        eng.stagger = stagger
        losses = []
        for _ in range(4):          # iteration 1 runs on one stream; 2-4 on the schedule under test
            q = [m_new, m_old]
            student.mask_provider = lambda n: q.pop(0)
            total, ce, kld = eng.iteration(images, labels, images if pipelined else None)
            losses.append((float(ce), float(kld)))
        torch.cuda.synchronize()
        assert eng.multi_stream
        bufs = torch.cat([b.detach().float().flatten() for b in student.buffers()])
        return losses, eng.optimizer.flat_param.clone(), bufs

    ref = run(None, False)
    for stagger, pipelined in ((0, False), (8, False), (8, True), (13, True), (99, False), (None, True)):
        got = run(stagger, pipelined)
        assert got[0] == ref[0], (stagger, pipelined, got[0], ref[0])
        assert torch.equal(got[1], ref[1]), (stagger, pipelined, float((got[1] - ref[1]).abs().max()))
        assert torch.equal(got[2], ref[2]), (stagger, pipelined)
