"""Fine-tuning / feature-extraction baseline, first increment (one old + one new decoder head) on
MI355X -- mirror of the reference's ``main_ftp1_enc_newbn.py``: flags (:466-498), checkpoint
loading with ``decoder -> decoder_old`` key remap (:213-221), freeze rule and optimizers
(:228-243), validation of the new and the old dataset every epoch (:318-324), 8-column
``automated_log.txt`` row (:359-361), file names (:339-344).  The hot loop is
``engine.FineTuneEngine``.  ``--synthetic N`` as in the other trainers."""
import os
import re
from argparse import ArgumentParser

import torch

from .dataset import ProceduralSeg, open_dataset
from .engine import FineTuneEngine
from .models.erfnet import NetFT1 as Net_ftp1
from .trainer_common import (CrossEntropyLoss2d, _strip, acc_or_neg_loss, add_common_flags,
                             class_weights, init_process, make_loader, run_epochs, validate,
                             write_model_txt)

NUM_CLASSES = 20
NUM_CLASSES_old = 20
NUM_CLASSES_new = 20
_init_dist = init_process          # process set-up only: no args, no savedir


def make_loaders(args, names_classes, new_index):
    """names_classes: [(dataset name, class count)] in task order -> (train loader of the new
    dataset, {name: val loader})."""
    val = {}
    for ind, (name, nc) in enumerate(names_classes):
        if args.synthetic:
            ds = ProceduralSeg(max(args.synthetic // 4, args.batch_size), args.height, args.width, nc,
                               seed=12 + ind, domain=ind)
        else:
            ds = open_dataset(name, "val", args, augment=False)
        val[name] = make_loader(ds, args, False, args.batch_size, False)
    name, nc = names_classes[new_index]
    if args.synthetic:
        tr = ProceduralSeg(args.synthetic, args.height, args.width, nc, seed=11, domain=new_index)
    else:
        tr = open_dataset(name, "train", args, augment=True)
    return make_loader(tr, args, True, args.batch_size, True), val


def finetune_epochs(args, model, engine, loader, num_classes_new, evaluate):
    """The epoch loop as both fine-tuning trainers run it (reference :253-361): scalars under
    'Finetuning_Baselines/runs_<model>_<epochs>_<batch><suffix>' like the reference's ``writer``
    (:109-111 / main_FT2_flexible_new.py:108-110), files tagged <model>_<epochs>_<batch>_<suffix>."""
    tag = "{}_{}_{}_{}".format(args.model, args.num_epochs, args.batch_size, args.model_name_suffix)
    writer_dir = "Finetuning_Baselines/runs_{}_{}_{}{}".format(
        args.model, args.num_epochs, args.batch_size, args.model_name_suffix)
    return run_epochs(args, model, engine, [loader], tag, writer_dir, evaluate,
                      banner="----- TRAINING - EPOCH", lr_groups=1, step=engine.iteration,
                      num_classes=num_classes_new, iou_train=True)


def train(args, finetune=False):
    print("old dataset: ", args.dataset_old)
    print("new dataset: ", args.dataset_new)
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    model = Net_ftp1(NUM_CLASSES_old, NUM_CLASSES_new)
    if args.state:
        saved = torch.load(args.state, map_location="cpu", weights_only=False)["state_dict"]
        new = {re.sub("decoder", "decoder_old", k): v for k, v in saved.items()}       # :218-220
        model.load_state_dict(_strip(new), strict=False)
        print("\nLOADED SAVED CITYSCAPES ENC -> ENC, DECODER --> OLD_DECODER for finetuning "
              "multi-head model on {}\n".format(args.dataset_new))
    model.to(dev)
    print("args.finetune: ", args.finetune)
    weight = class_weights(args.dataset_new).to(dev)
    criterion = CrossEntropyLoss2d(weight)
    criterion_old = CrossEntropyLoss2d(class_weights(args.dataset_old).to(dev))
    loader, val = make_loaders(args, [(args.dataset_old, NUM_CLASSES_old),
                                      (args.dataset_new, NUM_CLASSES_new)], 1)
    engine = FineTuneEngine(model, weight, finetune,
                            lambda x: model(x, decoder_old=False, decoder_new=True))
    print("finetuning optimizer" if finetune else "non-finetuning optimizer")
    write_model_txt(args, model)

    def evaluate(ep):
        avg_train = float(ep.sums[0]) / max(ep.n_it, 1)
        print("----- VALIDATING - EPOCH", ep.epoch, "--current---")
        ln, an = eval(model, val[args.dataset_new], criterion, NUM_CLASSES_new, ep.epoch, task=1)
        print("----- VALIDATING - EPOCH", ep.epoch, "--old----")
        lo, ao = eval(model, val[args.dataset_old], criterion_old, NUM_CLASSES_old, ep.epoch, task=0)
        return {"scalars": {"train_loss": avg_train,                                    # :327-332
                            "val_loss_{}".format(args.dataset_new): ln, "val_accuracy_{}".format(args.dataset_new): an,
                            "val_loss_{}".format(args.dataset_old): lo, "val_accuracy_{}".format(args.dataset_old): ao},
                "current_acc": acc_or_neg_loss(ln, an), "val_acc": an,
                "row": "\n%d\t\t%.4f\t\t%.4f\t\t%.4f\t\t%.4f\t\t%.4f\t\t%.4f\t\t%.8f" % (   # :359-361
                    ep.epoch, avg_train, ln, lo, ep.iou_train, an, ao, ep.lr)}

    return finetune_epochs(args, model, engine, loader, NUM_CLASSES_new, evaluate)


def eval(model, dataset_loader, criterion, num_classes, epoch, task=1):
    """:365-409 -- task 1 = new decoder, task 0 = old decoder."""
    global NUM_CLASSES
    NUM_CLASSES = num_classes
    decoder_old, decoder_new = (False, True) if task == 1 else (True, False)
    print("num_classes: ", NUM_CLASSES, "decoder_old: ", decoder_old, "decoder_new: ", decoder_new)
    avg, iou_val, _ = validate(model, lambda x: model(x, decoder_old, decoder_new), dataset_loader,
                               criterion, num_classes)
    print("EPOCH IoU on VAL set: ", "{:0.2f}".format(iou_val * 100), "%")
    return avg, iou_val


def main(args):
    global NUM_CLASSES_old, NUM_CLASSES_new
    NUM_CLASSES_old, NUM_CLASSES_new = args.num_classes_old, args.num_classes_new
    init_process(args)
    print("====== FINETUNING TRAINING OF NEW_DECODER & SHARED ENCODER ========")
    model = train(args, args.finetune)
    print("========== TRAINING FINISHED ===========")
    return model


def build_parser():
    p = ArgumentParser()
    add_common_flags(p, "erfnet_ftp1", "Finetune-CStoBDD-final", datadir=False)
    p.add_argument("--dataset-old", default="cityscapes")
    p.add_argument("--dataset-new", default="BDD")
    p.add_argument("--num-classes-old", type=int, default=20)
    p.add_argument("--num-classes-new", type=int, default=20)
    p.add_argument("--finetune", action="store_true")
    return p


if __name__ == "__main__":
    main(build_parser().parse_args())
