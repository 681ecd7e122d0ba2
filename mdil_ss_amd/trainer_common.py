"""What the six trainer mirrors and ``evaluate.py`` share: loss / checkpoint utilities, process
set-up, the common flags, loader construction, the validation pass and the epoch loop.  Each trainer
module keeps what is specific to it -- model construction and checkpoint key remap, freeze rule,
engine, per-batch step, which splits are validated and when, scalar names, log row -- and hands the
lines of the reference's output that differ between trainers (banner spelling, how many learning
rates are printed) to ``run_epochs`` as data."""
import os
import time
from types import SimpleNamespace

import torch
import torch.distributed as dist
from torch.utils.data import DataLoader

from . import engine as _engine
from . import ops
from .dataset import add_datadir_flags, to_device_batch
from .iouEval import iouEval

# class weights hard-coded by the reference (train_new_task_step2.py:121-131), copied as data
WEIGHTS = {
    "IDD": [3.235635601598852, 6.76221624390441, 9.458242359884549, 9.446818215454014,
            9.947040673126763, 9.789672819856547, 9.476665808564432, 10.465565126694731,
            9.59189547383129, 7.637805282159825, 8.990899026692638, 9.26222234098628,
            10.265657138809514, 9.386517631614392, 8.357391489170013, 9.910382864314824,
            10.389977663948363, 8.997422571963602, 10.418070541191673, 10.483262606962834,
            9.511436923349441, 7.597725385711079, 6.1734896019878205, 9.787631041755187,
            3.9178330193378708, 4.417448652936843, 10.313160683418731],
    "BDD": [3.6525147483016243, 8.799815287822142, 4.781908267406055, 10.034828238618045,
            9.5567865464289, 9.645099012085169, 10.315292989325766, 10.163473632969513,
            4.791692009441432, 9.556915153488912, 4.142994047786311, 10.246903827488143,
            10.47145010979545, 6.006704177894196, 9.60620532303246, 9.964959813857726,
            10.478333987902301, 10.468010534454706, 10.440929141422366, 3.960822533003462],
    "cityscapes": [2.8159904084894922, 6.9874672455551075, 3.7901719017455604, 9.94305485286704,
                   9.77037625072462, 9.511470001589007, 10.310780572569994, 10.025305236316246,
                   4.6341256102158805, 9.561389195953845, 7.869695292372276, 9.518873463871952,
                   10.374050047877898, 6.662394711556909, 10.26054487392723, 10.28786101490449,
                   10.289883605859952, 10.405463349170795, 10.138502340710136, 5.131658171724055],
}
# --datasets name -> key of WEIGHTS (train_multi_task.py:158-175; the notebook says 'cityscapes')
WEIGHT_NAME = {"cityscapes": "cityscapes", "CS": "cityscapes", "BDD": "BDD", "IDD": "IDD"}


def class_weights(name):
    w = torch.tensor(WEIGHTS[name], dtype=torch.float32)
    w[-1] = 0            # ignore class carries zero weight (:133-135)
    return w


class CrossEntropyLoss2d(torch.nn.Module):
    """NLLLoss2d(weight)(log_softmax(outputs, 1), targets) (:84-92) as one fused HIP kernel."""

    def __init__(self, weight=None):
        super().__init__()
        self.weight = weight

    def forward(self, outputs, targets):
        w = self.weight
        if w is None:
            w = torch.ones(outputs.shape[1], device=outputs.device)
        return ops.cross_entropy2d(outputs, targets, w.to(outputs.device))


def _strip(sd):
    return {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}


def _prefixed(sd):
    return {"module." + k: v for k, v in sd.items()}


def _is_dist():
    return dist.is_available() and dist.is_initialized()


def _rank():
    return dist.get_rank() if _is_dist() else 0


def _world():
    return dist.get_world_size() if _is_dist() else 1


def save_checkpoint(state, is_best, filenameCheckpoint, filenameBest):
    torch.save(state, filenameCheckpoint)
    print("Saving model: ", filenameCheckpoint)
    if is_best:
        print("Saving model as best: ", filenameBest)
        torch.save(state, filenameBest)


def init_process(args=None):
    """One process per GPU: device from LOCAL_RANK, the RCCL group when WORLD_SIZE > 1 and, given
    ``args``, ../save/<savedir> with opts.txt (rank 0).  -> the device."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1 and not _is_dist():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=dev)
    if args is not None and _rank() == 0:
        savedir = f"../save/{args.savedir}"
        os.makedirs(savedir, exist_ok=True)
        with open(savedir + "/opts.txt", "w") as f:
            f.write(str(args))
    return dev


def write_model_txt(args, model):
    if _rank() == 0:
        with open(f"../save/{args.savedir}/model.txt", "w") as f:
            f.write(str(model))


def add_common_flags(p, model, suffix, datadir=True):
    """The flags every trainer of the reference has; ``model`` / ``suffix``: the defaults of --model /
    --model-name-suffix; main_ftp1_enc_newbn.py alone has no --datadir."""
    p.add_argument("--cuda", action="store_true", default=True)
    p.add_argument("--model", default=model)
    p.add_argument("--state")
    p.add_argument("--port", type=int, default=8097)
    if datadir:
        p.add_argument("--datadir", default=os.getenv("HOME", "") + "/datasets/cityscapes/")
    p.add_argument("--height", type=int, default=512)
    p.add_argument("--width", type=int, default=1024)
    p.add_argument("--num-epochs", type=int, default=150)
    p.add_argument("--num-workers", type=int, default=4)
    p.add_argument("--batch-size", type=int, default=6)
    p.add_argument("--steps-loss", type=int, default=50)
    p.add_argument("--steps-plot", type=int, default=50)
    p.add_argument("--epochs-save", type=int, default=0)
    p.add_argument("--savedir", required=True)
    p.add_argument("--decoder", action="store_true")
    p.add_argument("--pretrainedEncoder")
    p.add_argument("--iouTrain", action="store_true", default=False)
    p.add_argument("--iouVal", action="store_true", default=True)
    p.add_argument("--resume", action="store_true")
    p.add_argument("--model-name-suffix", default=suffix)
    p.add_argument("--synthetic", type=int, default=0,
                   help="train on N seeded procedural images (MI355X build extension)")
    add_datadir_flags(p)


def make_loader(ds, args, train, batch_size, drop_last, seed=0, shard=None, cache_classes=None):
    """DataLoader over ``ds``.  The training split is shuffled and, under data parallelism, sharded
    by a DistributedSampler seeded ``seed``: every rank must run the same number of iterations (one
    gradient exchange each), so the sampler pads the shuffled index list to a multiple of the world
    size.  ``shard`` (default: ``train``) on a validation split: rank r takes images r, r+world, ...
    without padding; the caller sums the counts over the ranks, so every image is scored exactly
    once.  ``cache_classes``: class count for the trainers that have the --cache-resized DIR
    --cache-device path -- the split's post-Resize bytes live in HBM; an epoch is a permutation +
    three draws per sample on the host, a gather + the augment kernel on the GPU."""
    world = _world()
    shard = train if shard is None else shard
    if cache_classes is not None and getattr(args, "cache_device", False) and not args.synthetic:
        if not getattr(args, "cache_resized", None):
            raise RuntimeError("--cache-device needs --cache-resized DIR")
        from .dataset import DeviceResizedCache
        dev = torch.device("cuda", torch.cuda.current_device())
        rank, world = (_rank(), world) if shard else (0, 1)
        return DeviceResizedCache(ds, dev, args.num_workers).loader(
            batch_size, cache_classes, train, drop_last, rank, world)
    sampler = None
    if world > 1 and train:
        sampler = torch.utils.data.distributed.DistributedSampler(ds, shuffle=True, seed=seed)
    elif world > 1 and shard:
        ds = torch.utils.data.Subset(ds, range(_rank(), len(ds), world))
    return DataLoader(ds, num_workers=args.num_workers, batch_size=batch_size,
                      shuffle=train and sampler is None, sampler=sampler, drop_last=drop_last)


def validate(model, forward, loader, criterion, num_cls, sum_ranks=False, check_labels=False,
             broadcast=True):
    """Validation pass: eval-mode ``forward(inputs)``, CE, fused argmax + confusion counts.
    ``broadcast``: score the model rank 0 checkpoints.  ``sum_ranks``: the validation images are
    sharded over the ranks (``make_loader(shard=True)``) -- sum the confusion counts and the loss
    over the shards -> the metric of the whole validation set on every rank.
    -> (mean loss, mIoU, per-class IoU)."""
    model.eval()
    if broadcast:
        _engine.broadcast_buffers(model)
    dev = next(model.parameters()).device
    meter = iouEval(num_cls, num_cls - 1)
    loss_sum, n = torch.zeros((), device=dev), 0
    with torch.no_grad():
        for batch in loader:
            inputs, targets = to_device_batch(batch, dev, num_cls)
            outputs = forward(inputs)
            loss_sum += criterion(outputs, targets[:, 0])
            n += 1
            meter.addBatch(outputs, targets)
    if sum_ranks and _world() > 1:
        if meter.counts is None:
            meter.counts = torch.zeros(3, num_cls, dtype=torch.int64, device=dev)
        dist.all_reduce(meter.counts, op=dist.ReduceOp.SUM)
        ln = torch.stack([loss_sum.double(), torch.tensor(float(n), dtype=torch.float64, device=dev)])
        dist.all_reduce(ln, op=dist.ReduceOp.SUM)
        loss_sum, n = ln[0], int(ln[1].item())
    iou_val, iou_classes = meter.getIoU()
    avg = float(loss_sum) / max(n, 1)
    if check_labels:
        ops.check_labels()      # raises like torch's device assert if a label was out of range
    return avg, float(iou_val), iou_classes


def acc_or_neg_loss(loss, acc):
    """The reference's best-model criterion: the mIoU, or minus the loss while the mIoU is 0."""
    return -loss if acc == 0 else acc


def run_epochs(args, model, engine, loaders, tag, writer_dir, evaluate, *, banner, lr_groups=None,
               step=None, num_classes=None, n_sums=1, iou_train=False, check_labels=False,
               epoch_time=True, body=None, best_txt=True):
    """The epoch loop of every trainer: LR schedule, training pass, ``evaluate``, TensorBoard
    scalars, best-model rule, checkpoint files, best.txt, automated_log.txt.

    Training pass: ``body(epoch) -> (loss sums, iterations)``, or the loop over ``loaders[0]`` with
    ``step(images, labels) -> loss`` (a device scalar, or ``n_sums`` of them stacked, the total
    first); with ``iou_train`` and --iouTrain the training logits are scored against the labels.
    ``evaluate(ep) -> dict``; ``ep``: epoch, sums, n_it, iou_train (0 when not scored), lr (the last
    one printed); the dict: ``scalars``, ``current_acc`` (best-model criterion), ``val_acc`` (for
    best.txt) and optionally ``row`` (this epoch's line of automated_log.txt).
    ``banner`` / ``lr_groups`` / ``epoch_time``: the spelling of the epoch banner, how many groups'
    learning rates are printed (None: all) and whether 'epoch took' is, per reference trainer."""
    from .scalar_log import add_scalars, close_writer, open_writer
    writer = open_writer(writer_dir, _rank())
    dev = next(model.parameters()).device
    savedir = f"../save/{args.savedir}"
    log_path = savedir + "/automated_log.txt"
    if _rank() == 0 and not os.path.exists(log_path):
        with open(log_path, "a") as f:
            f.write("Epoch\t\tTrain-loss\t\tTest-loss\t\tTrain-IoU\t\tTest-IoU\t\tlearningRate")
    optimizer = engine.optimizer
    best_acc = 0
    for epoch in range(1, args.num_epochs + 1):
        print(banner, epoch, "-----")
        optimizer.set_epoch(epoch, args.num_epochs)      # LambdaLR.step(epoch)
        ep = SimpleNamespace(epoch=epoch, iou_train=0)
        for g in optimizer.param_groups[:lr_groups]:
            print("LEARNING RATE: ", g["lr"])
            ep.lr = float(g["lr"])
        for loader in loaders:
            if hasattr(loader.sampler, "set_epoch"):
                loader.sampler.set_epoch(epoch)
        if body is not None:
            ep.sums, ep.n_it = body(epoch)
        else:
            meter = iouEval(num_classes, num_classes - 1) if iou_train and args.iouTrain else None
            ep.sums, ep.n_it, t0 = torch.zeros(n_sums, device=dev), 0, time.time()
            for i, batch in enumerate(loaders[0]):
                images, labels = to_device_batch(batch, dev, num_classes)
                ep.sums += step(images, labels)
                ep.n_it += 1
                if meter is not None:
                    meter.addBatch(engine.last_outputs, labels)
                if args.steps_loss > 0 and i % args.steps_loss == 0:
                    avg = float(ep.sums[0]) / ep.n_it           # the only host sync in the loop
                    if check_labels:
                        ops.check_labels()      # raises like torch's device assert if a label was out of range
                    print(f"loss: {avg:0.4} (epoch: {epoch}, step: {i})",
                          "// Avg time/img: %.4f s" % ((time.time() - t0) / ep.n_it / args.batch_size))
            if epoch_time:
                print("epoch took: ", time.time() - t0)
            if meter is not None:
                ep.iou_train = float(meter.getIoU()[0])
        res = evaluate(ep)
        add_scalars(writer, res["scalars"], epoch)
        is_best = res["current_acc"] > best_acc
        best_acc = max(res["current_acc"], best_acc)
        if _rank() == 0:
            save_checkpoint({
                "epoch": epoch + 1, "arch": str(model),
                "state_dict": _prefixed(model.state_dict()),
                "best_acc": best_acc, "optimizer": optimizer.state_dict(),
            }, is_best, savedir + f"/checkpoint_{tag}.pth.tar", savedir + f"/model_best_{tag}.pth.tar")
            if is_best and best_txt:
                with open(savedir + "/best.txt", "w") as f:
                    f.write("Best epoch is %d, with Val-IoU= %.4f" % (epoch, res["val_acc"]))
            if "row" in res:
                with open(log_path, "a") as f:
                    f.write(res["row"])
    close_writer(writer)
    return model
