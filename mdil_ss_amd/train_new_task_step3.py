"""Step-3 incremental trainer (third domain, two old domains distilled) on MI355X.

Mirrors ``train_new_task_step3.py`` of the reference: ``is_shared`` / ``is_DS_curr`` (:88-101),
the freeze rule (:229-241), the two-step hot loop (:303-356, ``engine.Step3Engine``), validation
of every dataset in ``--datasets`` at epoch 1 and every 10th epoch (:392-399), checkpoint naming
(:436-451) and the CLI (:606-651: ``--dataset-new``, ``--datasets`` replace step 2's
``--dataset`` / ``--dataset_old``).  ``eval`` takes the class count of the validated task as an
int here, as in that file (:464).

Deliberate differences: ``--synthetic N`` procedural data (no datasets offline); one process per
GPU + RCCL instead of DataParallel over devices [0,1,2] with the old model on device 3 (:497-498);
the per-iteration ``.item()`` calls are replaced by a host read every ``--steps-loss`` iterations.
The epoch-wise tensorboard scalars (:424-425) are written as event files (``scalar_log``).
"""
from argparse import ArgumentParser

import torch

from .dataset import ProceduralSeg, open_dataset
from .engine import Step3Engine
from .models.erfnet_RA_parallel import Net as Net_RAP
from .train_new_task_step2 import apply_step2_freeze, is_shared, student_init_dict  # same rules, :229-241
from .trainer_common import (CrossEntropyLoss2d, _prefixed, _strip, acc_or_neg_loss, add_common_flags,
                             class_weights, init_process, make_loader, run_epochs, validate, write_model_txt)

NUM_CLASSES = 27
current_task = 2


def is_DS_curr(n):
    t = current_task
    if "decoder.{}".format(t) in n:
        return True
    if "encoder" in n and ("bn" in n or "parallel_conv" in n):
        return ".{}.weight".format(t) in n or ".{}.bias".format(t) in n
    return False


def make_loaders(args):
    t = args.datasets.index(args.dataset_new)
    if args.synthetic:
        tr = ProceduralSeg(args.synthetic, args.height, args.width, args.num_classes[t], seed=11,
                           domain=t)
    else:                                   # reference :155-171
        tr = open_dataset(args.dataset_new, "train", args, augment=True)
    loader = make_loader(tr, args, True, args.batch_size, True, cache_classes=args.num_classes[t])
    loader_val = {}
    for ind, d in enumerate(args.datasets):
        if args.synthetic:
            va = ProceduralSeg(max(args.synthetic // 4, args.batch_size), args.height, args.width,
                               args.num_classes[ind], seed=12 + ind, domain=ind)
        else:                               # reference :196-212
            va = open_dataset(d, "val", args, augment=False)
        # every rank scores the whole set here
        loader_val[d] = make_loader(va, args, False, args.batch_size, False,
                                    cache_classes=args.num_classes[ind])
    return loader, loader_val


def train(args, model, model_old):
    global NUM_CLASSES
    NUM_CLASSES = n_cls = args.num_classes[args.current_task]
    dev = next(model.parameters()).device
    criterion_val = {d: CrossEntropyLoss2d(class_weights(d).to(dev))
                     for d in ("cityscapes", "IDD", "BDD")}
    weight = criterion_val[args.dataset_new].weight
    loader, loader_val = make_loaders(args)
    print("global current_task: ", current_task)
    apply_step2_freeze(model, model_old, current_task)
    write_model_txt(args, model)
    engine = Step3Engine(model, model_old, weight, current_task=current_task,
                         lambdac=args.lambdac, is_shared=is_shared, is_ds_curr=is_DS_curr,
                         teacher_train=not args.eval_teacher, legacy_zero_grad=args.legacy_zero_grad)

    def step(images, labels):
        ce, kld_prev1, kld_prev0 = engine.iteration(images, labels)
        kd = args.lambdac * (kld_prev1 + kld_prev0)
        return torch.stack([ce + kd, ce, kd])                       # :358-360

    def evaluate(ep):
        average_loss_val = {d: 0.0 for d in args.datasets}
        val_acc = {d: 0.0 for d in args.datasets}
        if ep.epoch == 1 or ep.epoch % 10 == 0:
            print("----- VALIDATING - EPOCH", ep.epoch, "-----")
            for ind, d in enumerate(args.datasets):
                print("validate: ", d)
                average_loss_val[d], val_acc[d] = eval(model, loader_val[d], criterion_val[d], ind,
                                                       args.num_classes[ind], ep.epoch)
        info = {}
        for d in args.datasets:
            info["val_acc_{}".format(d)] = val_acc[d]
            info["val_loss_{}".format(d)] = average_loss_val[d]
        print(info)
        new = args.dataset_new
        return {"scalars": info, "val_acc": val_acc[new],                   # :425-426
                "current_acc": acc_or_neg_loss(average_loss_val[new], val_acc[new])}

    tag = "{}_{}_{}_{}{}_step{}".format(args.dataset_new, args.model, args.num_epochs,
                                        args.batch_size, args.model_name_suffix,
                                        len(args.num_classes))
    return run_epochs(args, model, engine, [loader], tag, "Adaptations/runs_" + tag, evaluate,   # :116-118
                      banner="-----TRAINING - EPOCH---", step=step, num_classes=n_cls, n_sums=3,
                      check_labels=True)


def eval(model, dataset_loader, criterion, task, num_classes, epoch):
    """Validation pass (:464-504); ``num_classes`` is the class count of ``task``."""
    global NUM_CLASSES
    NUM_CLASSES = num_classes
    print("number of classes in current task: ", num_classes)
    print("validating task: ", task)
    avg, iou_val, _ = validate(model, lambda x: model(x, task), dataset_loader, criterion, num_classes,
                               check_labels=True)
    print("EPOCH IoU on VAL set: ", "{:0.2f}".format(iou_val * 100), "%")
    print("check val fn, loss, acc: ", avg, iou_val)
    return avg, iou_val


def main(args):
    global current_task
    current_task = args.current_task
    print("\ndataset: ", args.dataset_new)
    dev = init_process(args)
    assert args.model == "erfnet_RA_parallel", "Error: model definition not found"
    print(args.num_classes, args.num_classes_old, args.nb_tasks, args.dataset_new)
    model = Net_RAP(args.num_classes, args.nb_tasks, args.current_task)
    model_old = Net_RAP(args.num_classes_old, args.nb_tasks - 1, args.current_task - 1)
    if args.state:
        saved = torch.load(args.state, map_location="cpu")["state_dict"]
        model_old.load_state_dict(_strip(saved), strict=False)
        print("loading previous step weights - CS-RAPs, BDD-RAPs and shared weights from previous step.")
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
    p.add_argument("--dataset-new", default="IDD")
    p.add_argument("--datasets", nargs="+", required=True, default=["IDD", "CS", "BDD"],
                   help="pass list of datasets in order")
    p.add_argument("--num-classes", type=int, nargs="+", required=True, default=[20, 20, 27])
    p.add_argument("--num-classes-old", type=int, nargs="+", required=True, default=[20])
    p.add_argument("--nb_tasks", type=int, default=3)
    p.add_argument("--current_task", type=int, default=2)
    p.add_argument("--lambdac", type=float, default=0.1)
    p.add_argument("--eval-teacher", action="store_true",
                   help="run the previous model in eval mode (the reference leaves it in train mode)")
    p.add_argument("--legacy-zero-grad", action="store_true",
                   help="torch<=1.x zero_grad semantics: the DS group also steps after the KD backward")
    return p


if __name__ == "__main__":
    main(build_parser().parse_args())
