"""Command line entry of the SVG baseline with the reference's flags (main_svg.py of the reference: same names, types,
defaults and choices), so a job script written for the reference drives this implementation unchanged.  Additions, as
main_srnn.py has them (all optional):
  --synthetic_data   use the built-in SM-MNIST-shaped generator instead of files on disk;
  --max_steps        stop after that many optimizer steps;
  --mnist_root       where `--choose_data mnist` reads the MNIST digits (never downloaded);
  --data_seed        keys the random draws of Stochastic Moving MNIST and the clip choice of BAIR / KTH;
  --data_root        where `--choose_data bair` / `kth` read their files;
  --data_cache       directory for the packed frame stores of BAIR / KTH.
One documented deviation: --variance.  The reference's SVG.__init__ reads `args.variance`, and its own parser never
defines it, so the reference's main_svg.py cannot construct the model as it stands; here the flag exists (default 1.0).
One GPU, eager steps: `--multigpu` is refused (SVG/trainer.py)."""
import argparse

from main_rfn import add_bool_arg, restricted_float


def build_parser():
    p = argparse.ArgumentParser()
    # DATA
    p.add_argument("--batch_size", help="Specify batch size", default=100, type=int)
    p.add_argument("--n_frames", help="Specify number of frames", default=10, type=int)
    p.add_argument("--choose_data", help="Specify dataset", choices=["mnist", "bair", "kth"], default="mnist", type=str)
    p.add_argument("--image_size", help="Specify the image size of mnist", default=64, type=int)
    p.add_argument("--digit_size", help="Specify the size of mnist digit", default=32, type=int)
    p.add_argument("--step_length", help="Specify the step size of mnist digit", default=4, type=int)
    p.add_argument("--num_digits", help="Specify the number of mnist digits", default=2, type=int)
    p.add_argument("--num_workers", help="Specify the number of workers in dataloaders", default=4, type=int)
    add_bool_arg(p, "use_validation_set", default=False, help="Specify if we want to use a validation set")
    # Trainer
    p.add_argument("--patience_es", help="Specify patience for early stopping", default=50, type=int)
    p.add_argument("--patience_lr", help="Specify patience for lr_scheduler", default=20, type=int)
    p.add_argument("--factor_lr", help="Specify lr_scheduler factor (0..1)", default=0.5, type=restricted_float)
    p.add_argument("--min_lr", help="Specify minimum lr for scheduler", default=0.0001, type=float)
    p.add_argument("--n_bits", help="Specify number of bits", default=8, type=int)
    p.add_argument("--n_epochs", help="Specify number of epochs", default=200, type=int)
    add_bool_arg(p, "verbose", default=False, help="Specify verbose mode (boolean)")
    p.add_argument("--path", help="Specify path to experiment", default="/content/", type=str)
    p.add_argument("--learning_rate", help="Specify learning_rate", default=0.001, type=float)
    p.add_argument("--preprocess_range", help="Specify the range of the data for preprocessing",
                   choices=["0.5", "1.0", "minmax", "none"], default="none", type=str)
    p.add_argument("--preprocess_scale", help="Specify the scale for preprocessing", default=255, type=int)
    p.add_argument("--beta_max", help="Specify the maximum value of beta", default=0.0001, type=float)
    p.add_argument("--beta_min", help="Specify the minimum value of beta", default=0.0001, type=float)
    p.add_argument("--beta_steps", help="Specify the annealing steps", default=1, type=int)
    p.add_argument("--n_predictions", help="Specify number of predictions", default=5, type=int)
    p.add_argument("--n_conditions", help="Specify number of conditions", default=5, type=int)
    add_bool_arg(p, "multigpu", default=False, help="Specify if we want to use multi GPUs")
    add_bool_arg(p, "load_model", default=False, help="Specify if we want to load a pre-existing model (boolean)")
    # SVG
    p.add_argument("--posterior_rnn_layers", help="Specify layers of posterier (variational encoder)", default=1, type=int)
    p.add_argument("--predictor_rnn_layers", help="Specify layers of predictor", default=2, type=int)
    p.add_argument("--prior_rnn_layers", help="Specify layers of variational prior", default=1, type=int)
    p.add_argument("--c_features", help="Specify channels of extracted features", default=256, type=int)
    p.add_argument("--x_dim", nargs="+", help="Specify data dimensions (b,c,h,w)", default=[100, 1, 64, 64], type=int)
    p.add_argument("--condition_dim", nargs="+", help="Specify condition dimensions (b,c,h,w)",
                   default=[100, 1, 64, 64], type=int)
    p.add_argument("--h_dim", help="Specify hidden state (h) channels", default=256, type=int)
    p.add_argument("--z_dim", help="Specify latent (z) channels", default=12, type=int)
    p.add_argument("--loss_type", help="Specify the type of loss used", default="mse",
                   choices=["bernoulli", "mse", "gaussian"], type=str)
    p.add_argument("--norm_type", help="Specify the type of loss used", default="batchnorm",
                   choices=["batchnorm", "instancenorm", "none"], type=str)
    add_bool_arg(p, "dequantize", default=True, help="Specify if we want to use uniform distribution for the loss")
    # a deviation from the reference's parser, which lacks it although its model reads args.variance
    p.add_argument("--variance", help="Scale of the Gaussian likelihood of --loss_type gaussian (the reference's model "
                   "reads args.variance, its parser never defines it)", default=1.0, type=float)
    # additions of this implementation (as in main_srnn.py)
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
    return p


def main(args):
    from SVG.trainer import Solver
    if args.load_model:
        # svg.pt may come from the reference: nothing from the file is executed
        ckpt = Solver.read_checkpoint("." + args.path + "model_folder/svg.pt")
        solver = Solver(ckpt["args"])
        solver.build()
        solver.load(ckpt)
    else:
        solver = Solver(args)
        solver.build()
    solver.train()


if __name__ == "__main__":
    main(build_parser().parse_args())
