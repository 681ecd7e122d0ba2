"""Step-2 incremental trainer (proposed method: RAP + domain-adaptive KD) on MI355X.

Mirrors the entry points, flags, file outputs and state-dict conventions of the reference's
``train_new_task_step2.py`` (prachigarg23/MDIL-SS): ``CrossEntropyLoss2d``, ``is_shared``,
``is_DS_curr``, ``train``, ``eval``, ``save_checkpoint``, ``main`` and the CLI of :541-587.
Underneath, the hot loop (:273-313) is ``engine.Step2Engine`` -- HIP kernels, one process per
GPU, RCCL gradient all-reduce -- instead of nn.DataParallel over ATen/cuDNN.

Differences that are deliberate (and flagged):
  * ``--synthetic N`` trains on the seeded procedural dataset (no dataset ships offline);
    ``--datadir`` style real loaders are a later row.
  * the per-iteration ``.item()`` x3 and ``torch.cuda.empty_cache()`` (:308-313) are replaced by
    a host read every ``--steps-loss`` iterations.
  * checkpoints keep the DataParallel ``module.`` key prefix so they interchange with the
    reference's (:441-446, :483-530).
"""
import re
from argparse import ArgumentParser

import torch

from .dataset import MyCoTransform, ProceduralSeg, open_dataset  # noqa: F401  (MyCoTransform: reference name)
from .engine import Step2Engine
from .models.erfnet_RA_parallel import Net as Net_RAP
from .trainer_common import (WEIGHTS, CrossEntropyLoss2d, class_weights, save_checkpoint,  # noqa: F401
                             _prefixed, _strip, _world, acc_or_neg_loss, add_common_flags,
                             init_process, make_loader, run_epochs, validate, write_model_txt)

NUM_CLASSES = 20
current_task = 0   # module global read by is_DS_curr, like the reference (:45,99-105)


def is_shared(n):
    return "encoder" in n and "parallel_conv" not in n and "bn" not in n


def is_DS_curr(n):
    t = current_task
    if "decoder.{}".format(t) in n:
        return True
    if "encoder" in n and ("bn" in n or "parallel_conv" in n):
        return ".{}.weight".format(t) in n or ".{}.bias".format(t) in n
    return False


def apply_step2_freeze(model, model_old, t):
    """Freeze rule of :202-215: the whole old model; in the student every decoder but ``t`` and
    every encoder bn / parallel_conv that is not domain ``t``'s weight / bias."""
    for p in model_old.parameters():
        p.requires_grad = False
    for name, p in model.named_parameters():
        if "decoder" in name:
            if "decoder.{}".format(t) not in name:
                p.requires_grad = False
        elif "encoder" in name and ("bn" in name or "parallel_conv" in name):
            if not (".{}.weight".format(t) in name or ".{}.bias".format(t) in name):
                p.requires_grad = False


def student_init_dict(saved, student_keys, t):
    """Initialisation of the step-``t`` student from the step-(t-1) checkpoint (:497-530):
    common keys as they are; encoder DS(t-1) weight/bias -> DS(t) (running stats are NOT
    copied); decoder(t-1) -> decoder(t) except output_conv."""
    new = {k: v for k, v in saved.items() if k in student_keys}
    prev_w, prev_b = ".{}.weight".format(t - 1), ".{}.bias".format(t - 1)
    for k, v in saved.items():
        if "encoder" in k:
            if "parallel_conv" in k or "bn" in k:
                if prev_w in k:
                    new[re.sub(prev_w, ".{}.weight".format(t), k)] = v
                elif prev_b in k:
                    new[re.sub(prev_b, ".{}.bias".format(t), k)] = v
        elif "decoder" in k and "output_conv" not in k:
            new[re.sub("decoder.{}".format(t - 1), "decoder.{}".format(t), k)] = v
    return new


def make_loaders(args):
    n_cls = args.num_classes[args.current_task]
    # the old-domain validation set is scored as TASK 0 (eval(..., 0, ...) below, reference :343-347):
    # its ignore label is relabelled to THAT head's last class -- whatever current_task is
    n_old = args.num_classes[0]
    world = _world()
    dom, dom_old = args.current_task, max(args.current_task - 1, 0)
    if args.synthetic:
        tr = ProceduralSeg(args.synthetic, args.height, args.width, n_cls, seed=11, domain=dom)
        va = ProceduralSeg(max(args.synthetic // 4, args.batch_size), args.height, args.width, n_cls,
                           seed=12, domain=dom)
        vo = ProceduralSeg(max(args.synthetic // 4, args.batch_size), args.height, args.width, n_old,
                           seed=13, domain=dom_old)
    else:                                   # reference :136-181
        tr = open_dataset(args.dataset, "train", args, augment=True)
        va = open_dataset(args.dataset, "val", args, augment=False)
        old = getattr(args, "dataset_old", None)            # the step-1 trainer has no old dataset
        vo = open_dataset(old, "val", args, augment=False) if old else va
    per_rank = args.batch_size
    if world > 1 and getattr(args, "dp_global_batch", False):
        # nn.DataParallel semantics: --batch-size is the GLOBAL batch, scattered over the GPUs
        assert args.batch_size % world == 0, "--dp-global-batch needs --batch-size divisible by the world size"
        per_rank = args.batch_size // world
    # the last, smaller batch of an epoch is trained on, as in the reference (:150-152: no
    # drop_last); under data parallelism it is dropped so that ranks stay in step.  Validation is
    # sharded over the ranks; eval() sums the counts
    loader = make_loader(tr, args, True, per_rank, world > 1, cache_classes=n_cls)
    loader_val = make_loader(va, args, False, args.batch_size, False, shard=True, cache_classes=n_cls)
    if vo is va:                            # step 1: one validation set, one resident copy
        return loader, loader_val, loader_val
    return loader, loader_val, make_loader(vo, args, False, args.batch_size, False, shard=True,
                                           cache_classes=n_old)


def train(args, model, model_old):
    global NUM_CLASSES
    NUM_CLASSES = n_cls = args.num_classes[args.current_task]    # of every training epoch (:251)
    dev = next(model.parameters()).device
    weight = class_weights(args.dataset).to(dev)
    criterion = CrossEntropyLoss2d(weight)
    criterion_old = CrossEntropyLoss2d(class_weights(args.dataset_old).to(dev))
    loader, loader_val, loader_val_old = make_loaders(args)

    apply_step2_freeze(model, model_old, current_task)
    write_model_txt(args, model)
    engine = Step2Engine(model, model_old, weight, current_task=current_task,
                         lambdac=args.lambdac, is_shared=is_shared, is_ds_curr=is_DS_curr,
                         global_ce=getattr(args, "dp_global_batch", False))
    engine.want_logits = bool(args.iouTrain)     # only --iouTrain reads the training logits (:317-320)

    def evaluate(ep):
        avg_total, avg_ce, avg_kld = (ep.sums / max(ep.n_it, 1)).tolist()
        if args.iouTrain:                                          # :329-333
            print("EPOCH IoU on TRAIN set: ", "{:0.2f}".format(ep.iou_train * 100), "%")
        print("----- VALIDATING - EPOCH", ep.epoch, "-----")
        loss_val, val_acc = eval(model, loader_val, criterion, current_task, args.num_classes, ep.epoch)
        loss_val_old, val_acc_old = eval(model, loader_val_old, criterion_old, 0, args.num_classes,
                                         ep.epoch)
        print("old-task loss and acc: ", loss_val_old, val_acc_old)
        return {"scalars": {"total_train_loss": avg_total, "KLD_loss_train": avg_kld, "ce_loss_train": avg_ce,
                            f"val_loss_{args.dataset}": loss_val, f"val_acc_{args.dataset}": val_acc,
                            f"val_loss_{args.dataset_old}": loss_val_old,
                            f"val_acc_{args.dataset_old}": val_acc_old},   # :351-355: epoch-wise scalars
                "current_acc": acc_or_neg_loss(loss_val, val_acc), "val_acc": val_acc,
                "row": "\n%d\t\t%.4f\t\t%.4f\t\t%.4f\t\t%.4f\t\t%.8f" % (
                    ep.epoch, avg_total, loss_val, ep.iou_train, val_acc, ep.lr)}

    tag = "{}_{}_{}_{}{}_step{}".format(args.dataset, args.model, args.num_epochs, args.batch_size,
                                        args.model_name_suffix, len(args.num_classes))
    # :115-117: SummaryWriter('Adaptations/runs_...'); LambdaLR.step(epoch), :244-254
    return run_epochs(args, model, engine, [loader], tag, "Adaptations/runs_" + tag, evaluate,
                      banner="-----TRAINING - EPOCH---", num_classes=n_cls, n_sums=3, iou_train=True,
                      check_labels=True, step=lambda images, labels: torch.stack(engine.iteration(images, labels)))


def eval(model, dataset_loader, criterion, task, num_classes, epoch):
    """Validation pass (:398-438) on this rank's shard of the set, summed over the ranks."""
    global NUM_CLASSES
    NUM_CLASSES = num_classes[task]
    avg, iou_val, _ = validate(model, lambda x: model(x, task), dataset_loader, criterion, NUM_CLASSES,
                               sum_ranks=True, check_labels=True)
    print("EPOCH IoU on VAL set: ", "{:0.2f}".format(iou_val * 100), "%")
    return avg, iou_val


def main(args):
    global current_task
    current_task = args.current_task
    dev = init_process(args)
    assert args.model == "erfnet_RA_parallel", "Error: model definition not found"
    model = Net_RAP(args.num_classes, args.nb_tasks, args.current_task)
    model_old = Net_RAP(args.num_classes_old, args.nb_tasks - 1, args.current_task - 1)
    if args.state:
        saved = torch.load(args.state, map_location="cpu")["state_dict"]
        model_old.load_state_dict(_strip(saved), strict=False)
        print("loading previous step weights - {}-RAPs and shared weights from previous step."
              .format(args.dataset_old))
        keys = {"module." + k for k in model.state_dict()}
        saved = saved if any(k.startswith("module.") for k in saved) else _prefixed(saved)
        model.load_state_dict(_strip(student_init_dict(saved, keys, current_task)), strict=False)
        print("loaded model from checkpoint provided.")
    model.to(dev)
    model_old.to(dev)
    model = train(args, model, model_old)
    print("========== TRAINING FINISHED ===========")
    return model


def build_parser():
    p = ArgumentParser()
    add_common_flags(p, "erfnet_RA_parallel", "RAPFT_KLD")
    p.add_argument("--dataset", default="cityscapes")
    p.add_argument("--dataset_old", default="IDD")
    p.add_argument("--num-classes", type=int, nargs="+", required=True, default=[20])
    p.add_argument("--num-classes-old", type=int, nargs="+", required=True, default=[20])
    p.add_argument("--nb_tasks", type=int, default=1)
    p.add_argument("--current_task", type=int, default=0)
    p.add_argument("--lambdac", type=float, default=0.1)
    p.add_argument("--dp-global-batch", action="store_true",
                   help="data parallel: treat --batch-size as the GLOBAL batch (scattered over the "
                        "GPUs like nn.DataParallel, BN over batch-size/world images per GPU) and take "
                        "the cross entropy as one weighted mean over the whole batch; default: "
                        "--batch-size images per GPU (BASELINE: 'batch 6/GPU'), rank-mean of per-shard "
                        "weighted means")
    return p


if __name__ == "__main__":
    main(build_parser().parse_args())
