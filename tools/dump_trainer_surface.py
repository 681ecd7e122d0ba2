#!/usr/bin/env python3
"""tests/golden/trainer_surface.json: the public surface of the six trainers and evaluate.py --
every parser action (option strings, dest, default, type, nargs, required, action class), the
signatures of the entry points and the names other code imports from them.  Needs no GPU.

    python tools/dump_trainer_surface.py > tests/golden/trainer_surface.json

The fixture is recorded from the commit BEFORE a change to the trainers and compared against the
commit after it (tests/test_trainer_surface_cpu.py), so regenerate it only when the surface is meant
to change.  ``--datadir`` defaults to $HOME/datasets/cityscapes/ and the dataset roots / cache
directory read MDIL_* variables: ``pin_environment`` fixes them."""
import importlib
import inspect
import json
import os
import sys

MODULES = ("train_RAPFT_step1", "train_new_task_step2", "train_new_task_step3", "train_multi_task",
           "main_ftp1_enc_newbn", "main_FT2_flexible_new", "evaluate")
FUNCTIONS = ("build_parser", "main", "train", "eval", "make_loaders")
NAMES = {
    "train_RAPFT_step1": ("apply_step1_freeze", "NUM_CLASSES"),
    "train_new_task_step2": ("is_shared", "is_DS_curr", "apply_step2_freeze", "student_init_dict",
                             "class_weights", "CrossEntropyLoss2d", "save_checkpoint", "WEIGHTS",
                             "MyCoTransform", "NUM_CLASSES", "current_task"),
    "train_new_task_step3": ("is_shared", "is_DS_curr", "NUM_CLASSES", "current_task"),
    "train_multi_task": ("is_shared", "is_DS_curr", "NUM_CLASSES", "current_task"),
    "main_ftp1_enc_newbn": ("run_epochs", "add_common_flags", "_init_dist", "NUM_CLASSES",
                            "NUM_CLASSES_old", "NUM_CLASSES_new"),
    "main_FT2_flexible_new": ("NUM_CLASSES",),
    "evaluate": (),
}


def pin_environment(setenv=os.environ.__setitem__, delenv=lambda k: os.environ.pop(k, None)):
    setenv("HOME", "/home/user")
    for k in ("MDIL_CS_DATADIR", "MDIL_BDD_DATADIR", "MDIL_IDD_DATADIR", "MDIL_CACHE_RESIZED"):
        delenv(k)


def surface():
    out = {}
    for name in MODULES:
        m = importlib.import_module("mdil_ss_amd." + name)
        actions = [{"option_strings": list(a.option_strings), "dest": a.dest, "default": a.default,
                    "type": getattr(a.type, "__name__", None), "nargs": a.nargs,
                    "required": a.required, "action": type(a).__name__}
                   for a in m.build_parser()._actions]
        out[name] = {
            "actions": sorted(actions, key=lambda a: a["dest"]),      # the order within --help is free
            "signatures": {f: str(inspect.signature(getattr(m, f))) for f in FUNCTIONS if hasattr(m, f)},
            "names": sorted(n for n in NAMES[name] if hasattr(m, n)),
        }
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    pin_environment()
    json.dump(surface(), sys.stdout, indent=1, sort_keys=True)
    print()
