#!/usr/bin/env python3
"""Write the Polyak-averaged weights of a run trained with --ema_decay as a run of their own, so that the evaluation
driver compares raw and averaged weights the way it compares any two experiments:

    python tools/export_ema.py --folder_path ./runs/ --experiment_names my_run [--out my_run_ema]
    python recurrent-flows-msc_amd/evaluation_metrics/eval_settings.py --folder_path ./runs/ \
        --experiment_names my_run my_run_ema --label_names raw ema --temperatures 0.7 0.7

`<folder_path><out>/model_folder/` becomes a copy of the run's model folder.  In every checkpoint of it that holds
averages (`optimizer_state_dict["state"][i]["ema"]`, i counting model.parameters()), `model_state_dict` holds the average
for each averaged parameter and the original value for everything else: buffers (BatchNorm running statistics, ActNorm
flags, ...) are never averaged, and a parameter that never saw a gradient has no average.  All other entries, the
optimizer state included, are the original's, so the copy loads through Solver.load like any checkpoint.  Files that
are not checkpoints (eval_dict.pt, status.txt) are copied as they are.  Nothing from a file is executed, and no GPU is
needed: the model is only constructed, from the stored arguments, to learn which state_dict entries are parameters."""
import argparse
import os
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "recurrent-flows-msc_amd"))
import torch


def export_ema(ckpt, param_keys):
    """a copy of the checkpoint dict `ckpt` whose model_state_dict holds the averaged weights.  `param_keys`: for every
    parameter of model.parameters(), in order (the optimizer's parameter indices), its state_dict key, or the tuple of
    its keys where modules share it (see `param_keys_of`).  Same top-level keys; the input is not modified.  ValueError
    when the checkpoint holds no average or an average does not fit its parameter."""
    from RFN.trainer import Solver
    emas = Solver.ema_tensors(ckpt)
    sd = dict(ckpt["model_state_dict"])
    for i, ema in sorted(emas.items()):
        if i >= len(param_keys):
            raise ValueError("the checkpoint averages parameter %d, the model has %d" % (i, len(param_keys)))
        keys = (param_keys[i],) if isinstance(param_keys[i], str) else tuple(param_keys[i])
        for name in keys:
            if name not in sd:
                raise ValueError("parameter %d (%s) is not in model_state_dict" % (i, name))
            if tuple(ema.shape) != tuple(sd[name].shape):
                raise ValueError("the average of %s has shape %s, the weights %s" %
                                 (name, tuple(ema.shape), tuple(sd[name].shape)))
            sd[name] = ema.detach().to(device=sd[name].device, dtype=sd[name].dtype).clone()
    out = dict(ckpt)
    out["model_state_dict"] = sd
    return out


def param_keys_of(model):
    """for every parameter of model.parameters(), in order, the tuple of its state_dict keys: a parameter that several
    modules share is listed once by parameters() but saved under each of its names, and load_state_dict copies them
    one after the other into the same tensor, so all of them must hold the average"""
    keys = {}
    for k, v in model.state_dict(keep_vars=True).items():
        keys.setdefault(id(v), []).append(k)
    return [tuple(keys[id(p)]) for p in model.parameters()]


def solver_for(file_name):
    """the Solver class whose train() writes a checkpoint of this name, or None"""
    import importlib
    for pkg in ("RFN", "SRNN", "VRNN", "SVG"):
        Solver = importlib.import_module(pkg + ".trainer").Solver
        if file_name in Solver.checkpoint_names:
            return Solver
    return None


def model_of(Solver, ckpt):
    """the model the checkpoint's arguments build (on the host; only its names are used)"""
    # the file describes the global batch; one process holds all of it
    return Solver(Solver.args_for_world(ckpt, 1)).make_model()


def export_folder(src, dst):
    """model folder `src` -> `dst`; returns the names of the checkpoints that were rewritten"""
    from RFN.trainer import Solver as RFNSolver
    os.makedirs(dst, exist_ok=True)
    done = []
    for name in sorted(os.listdir(src)):
        path = os.path.join(src, name)
        Solver = solver_for(name) if os.path.isfile(path) else None
        if Solver is not None:
            ckpt = RFNSolver.read_checkpoint(path)
            try:
                RFNSolver.ema_tensors(ckpt)
            except ValueError:
                Solver = None   # (e.g. a best-model file from before the flag was switched on: copied as it is)
        if Solver is None:
            if os.path.isfile(path):
                shutil.copyfile(path, os.path.join(dst, name))
            continue
        torch.save(export_ema(ckpt, param_keys_of(model_of(Solver, ckpt))), os.path.join(dst, name))
        done.append(name)
    if not done:
        raise ValueError("%s holds no checkpoint with averaged weights (train with --ema_decay)" % src)
    return done


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--folder_path", required=True, help="Folder holding the experiments (as for eval_settings.py)")
    ap.add_argument("--experiment_names", required=True, help="The run to export")
    ap.add_argument("--out", default=None, help="Name of the new experiment (default: <run>_ema)")
    a = ap.parse_args(argv)
    out = a.out or a.experiment_names + "_ema"
    src = os.path.join(a.folder_path, a.experiment_names, "model_folder")
    dst = os.path.join(a.folder_path, out, "model_folder")
    if os.path.abspath(src) == os.path.abspath(dst):
        raise ValueError("--out names the run itself")
    done = export_folder(src, dst)
    print("export_ema: %s -> %s (%s)" % (src, dst, ", ".join(done)))


if __name__ == "__main__":
    main()
