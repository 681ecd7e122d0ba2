"""Fine-tuning / feature-extraction baseline, second increment (two old decoder heads + a new one)
on MI355X -- mirror of the reference's ``main_FT2_flexible_new.py``: flags (:455-490), checkpoint
loading with ``decoder_old -> decoder_old1`` / ``decoder_new -> decoder_old2`` remap (:203-212),
freeze rule and optimizers (:220-235), validation of every dataset at epoch 1 and every 10th
(:305-311), file names (:335-340).  The reference imports ``models.erfnet_ft2``, which does not
exist in its tree; the model it means is ``models/erfnet_ftp2.py``.  Hot loop:
``engine.FineTuneEngine``."""
import os
import re
from argparse import ArgumentParser

import torch

from .engine import FineTuneEngine
from . import main_ftp1_enc_newbn as F1
from .models.erfnet import NetFT2 as Net_ft2
from .trainer_common import (WEIGHT_NAME, CrossEntropyLoss2d, _strip, acc_or_neg_loss, add_common_flags,
                             class_weights, init_process, validate, write_model_txt)

NUM_CLASSES = 27


def train(args, finetune=False):
    print("datasets: ", args.datasets)
    print("new dataset: ", args.dataset_new)
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    classes = args.num_classes
    model = Net_ft2(classes[0], classes[1], classes[2])
    if args.state:
        saved = torch.load(args.state, map_location="cpu", weights_only=False)["state_dict"]
        new = {}
        for k, v in saved.items():                                              # :205-211
            if "decoder_old" in k:
                k = re.sub("decoder_old", "decoder_old1", k)
            elif "decoder_new" in k:
                k = re.sub("decoder_new", "decoder_old2", k)
            new[k] = v
        model.load_state_dict(_strip(new), strict=False)
        print("\nLOADED SAVED CS-BDD ENC -> ENC, Dold->D1, Dnew->D2 for finetuning multi-head "
              "model on {}\n".format(args.dataset_new))
    model.to(dev)
    print("args.finetune: ", args.finetune)
    ce_loss = {d: CrossEntropyLoss2d(class_weights(WEIGHT_NAME[d]).to(dev)) for d in args.datasets}
    new_index = args.datasets.index(args.dataset_new)
    loader, val = F1.make_loaders(args, list(zip(args.datasets, classes)), new_index)
    engine = FineTuneEngine(model, ce_loss[args.dataset_new].weight, finetune,
                            lambda x: model(x, decoder_old1=False, decoder_old2=False, decoder_new=True))
    write_model_txt(args, model)

    def evaluate(ep):
        loss = {d: 0.0 for d in args.datasets}
        acc = {d: 0.0 for d in args.datasets}
        if ep.epoch % 10 == 0 or ep.epoch == 1:
            print("----- VALIDATING - EPOCH", ep.epoch)
            for ind, d in enumerate(args.datasets):
                print("validate: ", d)
                loss[d], acc[d] = eval(model, val[d], ce_loss[d], classes[ind], ep.epoch, ind)
        info = {}
        for d in args.datasets:
            info["val_acc_{}".format(d)] = acc[d]
            info["val_loss_{}".format(d)] = loss[d]
        print(info)
        new = args.dataset_new
        return {"scalars": info, "val_acc": acc[new],                            # :313-322
                "current_acc": acc_or_neg_loss(loss[new], acc[new])}

    return F1.finetune_epochs(args, model, engine, loader, classes[new_index], evaluate)


def eval(model, dataset_loader, criterion, num_classes, epoch, task=2):
    """:362-420 -- task 2 = new decoder, 1 = decoder_old2, 0 = decoder_old1."""
    global NUM_CLASSES
    NUM_CLASSES = num_classes
    flags = {2: (False, False, True), 1: (False, True, False), 0: (True, False, False)}[task]
    print("num_classes: ", NUM_CLASSES, "decoder_old1: ", flags[0], "decoder_old2: ", flags[1],
          "decoder_new: ", flags[2])
    avg, iou_val, _ = validate(model, lambda x: model(x, *flags), dataset_loader, criterion, num_classes)
    print("EPOCH IoU on VAL set: ", "{:0.2f}".format(iou_val * 100), "%")
    return avg, iou_val


def main(args):
    init_process(args)
    print("====== FINETUNING TRAINING OF NEW_DECODER & SHARED ENCODER ========")
    model = train(args, args.finetune)
    print("========== TRAINING FINISHED ===========")
    return model


def build_parser():
    p = ArgumentParser()
    add_common_flags(p, "erfnet_ftp2", "FE-CSBDDtoIDD-oldencBN")
    p.add_argument("--dataset-new", default="IDD")
    p.add_argument("--datasets", nargs="+", required=True, default=["IDD", "CS", "BDD"],
                   help="pass list of datasets in order")
    p.add_argument("--current_task", type=int, default=2)
    p.add_argument("--nb_tasks", type=int, default=3)
    p.add_argument("--num-classes", type=int, nargs="+", required=True, default=[20, 20, 27])
    p.add_argument("--finetune", action="store_true")
    return p


if __name__ == "__main__":
    main(build_parser().parse_args())
