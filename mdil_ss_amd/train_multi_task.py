"""Multi-task joint trainer (all domains at once, shared encoder + one head per domain) on MI355X.

Mirrors ``train_multi_task.py`` of the reference: ``is_shared`` / ``is_DS_curr`` (:107,110), the
optimizer groups (``5e-4/nb_tasks`` for the encoder, :212-220), the round-robin inner loop
(:249-265, ``engine.MultiTaskEngine``), validation of every dataset at epoch 1 and every 5th epoch
(:281-291), best-model rule on the mean IoU (:306-313), file names (:318-323) and the CLI
(:430-468).  The reference file does not import as shipped (``elif`` without ``if`` at :403); the
model selection below is what that line intends.  ``--synthetic N`` as in the other trainers.
"""
import re
import time
from argparse import ArgumentParser

import torch

from .dataset import ProceduralSeg, open_dataset, to_device_batch
from .engine import MultiTaskEngine
from .models.erfnet_multi_task import Net as Net_MT
from .trainer_common import (WEIGHT_NAME, CrossEntropyLoss2d, _strip, add_common_flags, class_weights,
                             init_process, make_loader, run_epochs, validate, write_model_txt)

NUM_CLASSES = 20
current_task = 0


def is_shared(n):
    return "encoder" in n


def is_DS_curr(n):
    return "decoder" in n


def make_loaders(args):
    loader_train, loader_val = {}, {}
    for ind, d in enumerate(args.datasets):
        if args.synthetic:
            tr = ProceduralSeg(args.synthetic, args.height, args.width, args.num_classes[ind],
                               seed=11 + 10 * ind, domain=ind)
            va = ProceduralSeg(max(args.synthetic // 4, 2), args.height, args.width,
                               args.num_classes[ind], seed=12 + 10 * ind, domain=ind)
        else:                               # reference :158-175
            tr = open_dataset(d, "train", args, augment=True)
            va = open_dataset(d, "val", args, augment=False)
        loader_train[d] = make_loader(tr, args, True, args.batch_size, False, seed=ind)
        loader_val[d] = make_loader(va, args, False, 2, True)
    return loader_train, loader_val


def train(args, model):
    print("datasets: ", args.datasets)
    print("nb_tasks: ", args.nb_tasks)
    print("dataset_name: ", args.dataset)
    print("num_classes: ", args.num_classes)
    dev = next(model.parameters()).device
    ce_loss = {d: CrossEntropyLoss2d(class_weights(WEIGHT_NAME[d]).to(dev)) for d in args.datasets}
    loader_train, loader_val = make_loaders(args)
    write_model_txt(args, model)
    print("\nusing learning rate this for the W_s params", 5e-4 / args.nb_tasks, "\n")
    print("using 5e-4 lr for W_t")
    engine = MultiTaskEngine(model, [ce_loss[d].weight for d in args.datasets])
    n_iters = min(len(loader_train[d]) for d in args.datasets)
    print("n_iters ", n_iters)

    def body(epoch):                                                        # :249-265
        global NUM_CLASSES
        iterator = {d: iter(loader_train[d]) for d in args.datasets}
        sums = torch.zeros(len(args.datasets), device=dev)
        t_epoch = time.time()
        model.train()
        for itr in range(n_iters):
            for ind, d in enumerate(args.datasets):
                NUM_CLASSES = args.num_classes[ind]
                images, labels = to_device_batch(next(iterator[d]), dev, NUM_CLASSES)
                sums[ind] += engine.sub_step(ind, images, labels)
        print("epoch took: ", time.time() - t_epoch)
        return sums, n_iters

    def evaluate(ep):
        average_loss_val = {d: 0.0 for d in args.datasets}
        val_acc = {d: 0.0 for d in args.datasets}
        if ep.epoch % 5 == 0 or ep.epoch == 1:
            for ind, d in enumerate(args.datasets):
                print("validate: ", d)
                average_loss_val[d], val_acc[d] = eval(model, loader_val[d], ce_loss[d], ind,
                                                       args.num_classes, ep.epoch)
        info = {}
        for i, d in enumerate(args.datasets):
            info["val_acc_{}".format(d)] = val_acc[d]
            info["val_loss_{}".format(d)] = average_loss_val[d]
            info["train_loss_{}".format(d)] = float(ep.sums[i]) / max(ep.n_it, 1)
        print(info)
        temp_acc = sum(val_acc[k] for k in args.datasets)                    # :306-313
        return {"scalars": info, "current_acc": -0.0 if temp_acc == 0 else temp_acc / len(args.datasets)}

    tag = "{}_{}_{}_{}{}_step{}".format(args.dataset, args.model, args.num_epochs, args.batch_size,
                                        args.model_name_suffix, len(args.num_classes))
    return run_epochs(args, model, engine, [loader_train[d] for d in args.datasets], tag,
                      "Adaptations/runs_" + tag, evaluate, banner="-----TRAINING - EPOCH---",   # :122-124
                      lr_groups=2, body=body, best_txt=False)


def eval(model, dataset_loader, criterion, task, num_classes, epoch):
    """Validation pass (:331-371); ``num_classes`` is the list, indexed by ``task``."""
    global NUM_CLASSES
    NUM_CLASSES = num_classes[task]
    print("number of classes in current task: ", NUM_CLASSES)
    print("validating task: ", task)
    avg, iou_val, _ = validate(model, lambda x: model(x, task), dataset_loader, criterion, NUM_CLASSES,
                               check_labels=True)
    print("EPOCH IoU on VAL set: ", "{:0.2f}".format(iou_val * 100), "%")
    print("check val fn, loss, acc: ", avg, iou_val)
    return avg, iou_val


def main(args):
    global current_task
    current_task = args.current_task
    print("\ndataset: ", args.dataset)
    dev = init_process(args)
    assert args.model == "erfnet_multi_task", "Error: model definition not found"
    print(args.num_classes, args.nb_tasks, args.dataset)
    model = Net_MT(args.num_classes, args.nb_tasks, args.current_task)
    if args.state:
        saved = torch.load(args.state, map_location="cpu")["state_dict"]
        print("loading ImageNet pre-trained enc")
        new = {re.sub("module.features", "module", k): v for k, v in saved.items()}   # :418-420
        model.load_state_dict(_strip(new), strict=False)
    print("loaded\n")
    model.to(dev)
    model = train(args, model)
    print("========== TRAINING FINISHED ===========")
    return model


def build_parser():
    p = ArgumentParser()
    add_common_flags(p, "erfnet_multi_task", "RAP_FT")
    p.add_argument("--dataset", default="CSBDD")
    p.add_argument("--datasets", nargs="+", required=True, default=["CS", "BDD"])
    p.add_argument("--dlr", type=float, default=100.0)
    p.add_argument("--num-classes", type=int, nargs="+", required=True, default=[20])
    p.add_argument("--nb_tasks", type=int, default=1)
    p.add_argument("--current_task", type=int, default=0)
    return p


if __name__ == "__main__":
    main(build_parser().parse_args())
