"""Step-1 trainer (first domain, RAP-FT model) on MI355X: mirror of the reference's
``train_RAPFT_step1.py`` for ``--model erfnet_RA_parallel`` -- same entry points (``train``, ``eval``,
``main``; ``save_checkpoint`` lives in ``trainer_common``), flags (:513-549), freeze rule
(:177-190), single-group Adam + poly LR (:260-272), checkpoint dict / file names, ``module.``-prefixed keys and the ImageNet-encoder key
remap (:482-491).  The hot loop is ``engine.Step1Engine`` (HIP kernels, one process per GPU,
RCCL gradient all-reduce).  The other ablation models of the reference trainer
(``erfnet_RA_series`` / ``erfnet_RCM`` / ``erfnet_bn`` / ``erfnet_onlyRAP``, :21-26) are not in this
repository and are refused explicitly."""
import re
from argparse import ArgumentParser

import torch

from . import train_new_task_step2 as S2
from .engine import Step1Engine
from .models.erfnet_RA_parallel import Net as Net_RAP
from .trainer_common import (CrossEntropyLoss2d, _strip, acc_or_neg_loss, add_common_flags, class_weights,
                             init_process, run_epochs, write_model_txt)

NUM_CLASSES = 20


def apply_step1_freeze(model, current_task):
    """:177-190 -- only decoder ``t`` and the encoder's domain-``t`` bn / parallel_conv weight+bias
    train among the domain-specific parameters; shared encoder convs always train."""
    for name, p in model.named_parameters():
        if "decoder" in name:
            p.requires_grad = "decoder.{}".format(current_task) in name
        elif "encoder" in name and ("bn" in name or "parallel_conv" in name):
            p.requires_grad = (".{}.weight".format(current_task) in name or
                               ".{}.bias".format(current_task) in name)


def eval(model, dataset_loader, criterion, task, num_classes, epoch):
    return S2.eval(model, dataset_loader, criterion, task, num_classes, epoch)


def train(args, model):
    global NUM_CLASSES
    t = args.current_task
    NUM_CLASSES = args.num_classes[t]
    dev = next(model.parameters()).device
    weight = class_weights(args.dataset).to(dev)
    criterion = CrossEntropyLoss2d(weight)
    loader, loader_val, _ = S2.make_loaders(args)      # same splits and sharding; no old dataset here
    apply_step1_freeze(model, t)
    write_model_txt(args, model)
    engine = Step1Engine(model, weight, current_task=t)

    def evaluate(ep):
        avg_train = float(ep.sums[0]) / max(ep.n_it, 1)
        print("----- VALIDATING - EPOCH", ep.epoch, "-----")
        loss_val, val_acc = eval(model, loader_val, criterion, t, args.num_classes, ep.epoch)
        return {"scalars": {"train_loss": avg_train, f"val_loss_{args.dataset}": loss_val,
                            f"val_acc_{args.dataset}": val_acc},                  # :340-344
                "current_acc": acc_or_neg_loss(loss_val, val_acc), "val_acc": val_acc,
                "row": "\n%d\t\t%.4f\t\t%.4f\t\t%.4f\t\t%.4f\t\t%.8f" % (
                    ep.epoch, avg_train, loss_val, 0, val_acc, ep.lr)}

    tag = "{}_{}_{}_{}{}_step{}".format(args.dataset, args.model, args.num_epochs, args.batch_size,
                                        args.model_name_suffix, len(args.num_classes))
    return run_epochs(args, model, engine, [loader], tag, "Adaptations/runs_" + tag, evaluate,   # :107-109
                      banner="----- TRAINING - EPOCH", lr_groups=1, step=engine.iteration,
                      num_classes=NUM_CLASSES, epoch_time=False)


def main(args):
    dev = init_process(args)
    if args.model != "erfnet_RA_parallel":
        raise SystemExit(f"model '{args.model}' is not part of the MI355X build (only erfnet_RA_parallel)")
    model = Net_RAP(args.num_classes, args.nb_tasks, args.current_task)
    if args.state:
        saved = torch.load(args.state, map_location="cpu")["state_dict"]
        if args.current_task == 0:
            print("loading ImageNet pre-trained enc")        # :482-491
            saved = {re.sub("module.features", "module", k): v for k, v in saved.items()}
        else:
            print("loading previous step weights")
        model.load_state_dict(_strip(saved), strict=False)
        print("loaded model from checkpoint provided.")
    model.to(dev)
    model = train(args, model)
    print("========== TRAINING FINISHED ===========")
    return model


def build_parser():
    p = ArgumentParser()
    add_common_flags(p, "erfnet_RA_parallel", "RAP_FT")
    p.add_argument("--dataset", default="cityscapes")
    p.add_argument("--num-classes", type=int, nargs="+", required=True, default=[20])
    p.add_argument("--nb_tasks", type=int, default=1)
    p.add_argument("--current_task", type=int, default=0)
    return p


if __name__ == "__main__":
    main(build_parser().parse_args())
