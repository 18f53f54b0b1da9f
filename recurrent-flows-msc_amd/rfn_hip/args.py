"""What the wrapper modules of this package share: the profiling metadata of a shell launch and the argument checks
that several wrappers make with the same words.  Every check names the calling function in its message (`who`)."""
import torch


def shape_label(t):
    """a tensor's shape as the `2x3x8x8` label of a launch's profiling metadata"""
    return "x".join(str(int(d)) for d in t.shape)


def shell(name, t, n_tensors):
    """profiling metadata of a memory-bound shell launch: algorithmic bytes = n_tensors x the tensor's fp32 size"""
    return ("shell", name, 0.0, shape_label(t), 4.0 * n_tensors * t.numel())


def flat(t):
    """the flat, detached, contiguous view of a parameter (None stays None)"""
    return None if t is None else t.detach().reshape(-1).contiguous()


def check_u63(who, **values):
    """every named integer is in [0, 2^63): a word of a noise key or a sequence id (checked in the order given)"""
    for nm, v in values.items():
        if not 0 <= v < 1 << 63:
            raise ValueError("%s: %s %d not in [0, 2^63)" % (who, nm, v))


def check_step(who, step):
    """the step word of a noise key is in [0, 2^31)"""
    if not 0 <= step < 1 << 31:
        raise ValueError("%s: step %d not in [0, 2^31)" % (who, step))


def fresh_device(who, device):
    """where the fresh tensors of `who` go: `device`, by default the current GPU; anything but a GPU is an error"""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("rfn_hip kernels need device tensors; %s was asked for %s (no CPU fallback)" % (who, device))
    return device
