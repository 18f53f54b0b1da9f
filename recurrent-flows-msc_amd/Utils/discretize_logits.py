"""Mixture of discretized logistics with the reference's names (Utils/discretize_logits.py of the reference, the
PixelCNN++ likelihood): `DiscretizedMixtureLogits(nr_mix)(logits=l)` gives an object with `.log_prob(value)` ([N,H,W]) and
`.sample()` ([N,C,H,W]), plus `.sample_keyed(...)`, the sampler with addressed uniforms.  All run on the HIP kernels
(rfn_hip.ops.mol_nll / mol_sample / mol_sample_keyed; DESIGN.md sections 19 and 20): device tensors only, gradient into
the logits only.  `DiscretizedMixtureLogits` is the RGB form (10 channels per component),
`DiscretizedMixtureLogits_1d` the one-channel form (3 per component)."""
from rfn_hip import ops as K


class _MixtureDistribution:
    channels = None

    def __init__(self, nr_mix, logits):
        per = 10 if self.channels == 3 else 3
        if logits.dim() != 4 or logits.shape[1] != per * nr_mix:
            raise RuntimeError("%s(nr_mix=%d) needs logits [N, %d, H, W], got %s" %
                               (type(self).__name__, nr_mix, per * nr_mix, tuple(logits.shape)))
        self.logits, self.nr_mix = logits, nr_mix

    def log_prob(self, value):
        return -K.mol_nll(value.detach(), self.logits, reduce="pixel")

    def sample(self, u_mix=None, u_x=None, generator=None):
        """u_mix [N,H,W,nr_mix], u_x [N,H,W,C]: recorded draws to replay (the reference draws them in this order)"""
        return K.mol_sample(self.logits, u_mix, u_x, generator=generator, channels=self.channels)

    def sample_keyed(self, B, seed, step, first_seq=0, first_draw=0):
        """`sample` with addressed uniforms (rfn_hip.ops.mol_sample_keyed): row r*B + b of the
        logits is draw first_draw + r of sequence first_seq + b.  No uniform tensor, torch's generator untouched."""
        return K.mol_sample_keyed(self.logits, B, seed, step, first_seq, first_draw, channels=self.channels)


class DiscretizedMixtureLogitsDistribution(_MixtureDistribution):
    channels = 3


class DiscretizedMixtureLogitsDistribution_1d(_MixtureDistribution):
    channels = 1


class DiscretizedMixtureLogits:
    distribution = DiscretizedMixtureLogitsDistribution

    def __init__(self, nr_mix, **kwargs):
        self.nr_mix = nr_mix

    def __call__(self, logits):
        return self.distribution(self.nr_mix, logits)


class DiscretizedMixtureLogits_1d(DiscretizedMixtureLogits):
    distribution = DiscretizedMixtureLogitsDistribution_1d
