"""Command line entry of the linear-extrapolation baseline (averagemodel/averagemodel.py of the reference, which is a
script with its settings as constants; the flags' defaults are those constants: 5 conditioning frames, test sequences of
20 frames, 10 predictions, batches of 256, 3 epochs, Adam at 1e-3).  Trains unless --load_model is given (then
`<path>model_folder/average.pt` is read), evaluates over the test loader and writes, under `<path>eval_folder/`:

  SSIM_PSNR_<data>_averagemodel_trained_on_<n+1>_frames.pt   the reference's file (:159-199): per test batch and predicted
      frame the batch means of pytorch_msssim's Gaussian-window SSIM and of the PSNR, on clamp(255 v, 0, 255) not
      rounded (rfn_hip.ops.gauss_quality): SSIM_values, PSNR_values [n_batches, P] and their means over the batches;
  evaluations.pt   the eleven keys of evaluation_metrics.eval_settings.eval_dict, so that Evaluator.plot_eval_values
      draws the baseline beside the other models (`--experiment_names my_run average_run`): SSIM / PSNR / MSE per
      sequence [N, P] by the Evaluator's own definitions (rfn_hip.ops.frame_quality on the uint8 frames
      clamp(255 v, 0, 255).byte()); the *_std_mean keys hold the same tensors (the model is deterministic: the mean over
      draws is the one draw); LPIPS entries are None unless --lpips_weights is given; temperature, BPD, DKL and RECON
      are None.

The data flags are those of main_svg.py (--synthetic_data, --mnist_root, --data_root, --data_cache, --data_seed, ...);
--max_steps stops the training early, --max_batches the evaluation.  One GPU."""
import argparse

import torch

from main_rfn import add_bool_arg


def build_parser():
    p = argparse.ArgumentParser()
    # DATA (main_svg.py's flags; the defaults that differ are the reference script's constants)
    p.add_argument("--batch_size", help="Specify batch size", default=256, type=int)
    p.add_argument("--n_frames", help="Specify number of frames of a test sequence", default=20, type=int)
    p.add_argument("--choose_data", help="Specify dataset", choices=["mnist", "bair", "kth"], default="bair", type=str)
    p.add_argument("--image_size", help="Specify the image size of mnist", default=64, type=int)
    p.add_argument("--digit_size", help="Specify the size of mnist digit", default=28, type=int)
    p.add_argument("--step_length", help="Specify the step size of mnist digit", default=4, type=int)
    p.add_argument("--num_digits", help="Specify the number of mnist digits", default=2, type=int)
    p.add_argument("--num_workers", help="Specify the number of workers in dataloaders", default=10, type=int)
    add_bool_arg(p, "use_validation_set", default=False, help="Specify if we want to use a validation set")
    p.add_argument("--x_dim", nargs="+", help="Specify data dimensions (b,c,h,w)", default=[256, 3, 64, 64], type=int)
    # Trainer
    p.add_argument("--n_epochs", help="Specify number of epochs", default=3, type=int)
    p.add_argument("--learning_rate", help="Specify learning_rate", default=0.001, type=float)
    p.add_argument("--path", help="Specify path to experiment", default="/content/", type=str)
    p.add_argument("--n_predictions", help="Specify number of predictions", default=10, type=int)
    p.add_argument("--n_conditions", help="Specify number of conditioning frames", default=5, type=int)
    add_bool_arg(p, "load_model", default=False, help="Evaluate <path>model_folder/average.pt instead of training")
    # additions of this implementation (as in main_svg.py)
    add_bool_arg(p, "synthetic_data", default=False, help="SM-MNIST-shaped synthetic video instead of files on disk")
    p.add_argument("--max_steps", help="Stop after this many optimizer steps (0 = no limit)", default=0, type=int)
    p.add_argument("--mnist_root", help="Directory holding torchvision's MNIST files for --choose_data mnist",
                   default="Mnist", type=str)
    p.add_argument("--data_seed", help="Seed of the Stochastic Moving MNIST sequences and of the BAIR / KTH clip choice",
                   default=0, type=int)
    p.add_argument("--data_root", help="Directory holding the files of --choose_data bair / kth (default: the "
                   "reference's, under the working directory)", default=None, type=str)
    p.add_argument("--data_cache", help="Directory for the packed frame stores of --choose_data bair / kth",
                   default=None, type=str)
    p.add_argument("--max_batches", help="Evaluate at most this many test batches", default=None, type=int)
    p.add_argument("--lpips_weights", nargs="+", help="Directory or files holding the LPIPS-alex weights (nothing is "
                   "downloaded); without it the LPIPS entries of evaluations.pt are None", default=None, type=str)
    return p


def reference_file_name(choose_data, n_conditions):
    """averagemodel.py:199"""
    return "SSIM_PSNR_%s_averagemodel_trained_on_%d_frames.pt" % (choose_data, n_conditions + 1)


def evaluate(solver, n_predictions, max_batches=None, lpips_weights=None):
    """(the reference's dict, the eval_dict-compatible dict) over solver.test_loader, as CPU tensors"""
    from rfn_hip import ops
    model = solver.model
    n, P = model.num_cond_frames, int(n_predictions)
    lpips_w = None
    if lpips_weights is not None:
        w = lpips_weights[0] if isinstance(lpips_weights, (list, tuple)) and len(lpips_weights) == 1 else lpips_weights
        lpips_w = ops.lpips_alex_load(w, solver.device)
    ssim_b, psnr_b, seq = [], [], {"ssim": [], "psnr": [], "mse": [], "lpips": []}
    with torch.no_grad():
        model.eval()
        for batch_i, image in enumerate(solver.test_loader):
            if max_batches is not None and batch_i >= max_batches:
                break
            image = solver.batch(image)
            B, T = int(image.shape[0]), int(image.shape[1])
            if T < n + P:
                raise ValueError("main_average: test sequences of %d frames cannot hold %d conditioning frames and %d "
                                 "predictions" % (T, n, P))
            pred = model.sample(image, P)
            true = image[:, n:n + P].contiguous()
            # the reference's figures (:174-183): per predicted frame, the batch mean over scaled, clamped, unrounded frames
            ssim, psnr, _ = ops.gauss_quality(pred.flatten(0, 1), true.flatten(0, 1), scale=255.0, lo=0.0, hi=255.0)
            ssim_b.append(ssim.view(B, P).mean(0))
            psnr_b.append(psnr.view(B, P).mean(0))
            # the Evaluator's figures (Evaluator.eval_seq): per sequence and frame, on uint8 frames
            pred_u8, true_u8 = (torch.clamp(255 * v, 0, 255).byte() for v in (pred, true))
            mse8, psnr8, ssim8 = ops.frame_quality(true_u8, pred_u8)
            seq["mse"].append(mse8)
            seq["psnr"].append(psnr8)
            seq["ssim"].append(ssim8)
            if lpips_w is not None:
                seq["lpips"].append(ops.lpips_alex_distance(lpips_w, ops.lpips_alex_features(lpips_w, pred_u8),
                                                            ops.lpips_alex_features(lpips_w, true_u8)))
    if not ssim_b:
        raise ValueError("main_average: the test loader yielded no batch")
    ssim_v, psnr_v = torch.stack(ssim_b).cpu(), torch.stack(psnr_b).cpu()
    reference = {"SSIM_values": ssim_v, "PSNR_values": psnr_v, "SSIM_values_mean": ssim_v.mean(0),
                 "PSNR_values_mean": psnr_v.mean(0)}
    cat = lambda k: torch.cat(seq[k]).cpu() if seq[k] else None
    mse, psnr, ssim, lpips = cat("mse"), cat("psnr"), cat("ssim"), cat("lpips")
    evaluations = {"SSIM_values": ssim, "PSNR_values": psnr, "MSE_values": mse, "LPIPS_values": lpips,
                   "temperature": None, "BPD": None, "DKL": None, "RECON": None,
                   "SSIM_std_mean": ssim, "PSNR_std_mean": psnr, "LPIPS_std_mean": lpips}
    return reference, evaluations


def main(args):
    from AverageModel.trainer import Solver
    solver = Solver(args)
    solver.build()
    if args.load_model:
        # nothing from the file is executed (Solver.read_checkpoint)
        solver.load(Solver.read_checkpoint(solver.path + "model_folder/average.pt"))
    else:
        solver.train()
    reference, evaluations = evaluate(solver, args.n_predictions, args.max_batches, args.lpips_weights)
    folder = solver.path + "eval_folder/"
    torch.save(reference, folder + reference_file_name(args.choose_data, args.n_conditions))
    torch.save(evaluations, folder + "evaluations.pt")
    return solver


if __name__ == "__main__":
    main(build_parser().parse_args())
