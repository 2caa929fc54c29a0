"""Learning-rate warmup and decay for the fused step (fabric_amd/train.py: --lr_warmup_updates, --lr_schedule, --lr_min).  Host only: the
schedule is a function of the UPDATE index, a Python int, and writes Python floats into `step.lr` and the step's param groups, which the
update reads at every call anyway -- nothing is launched and nothing waits for the device.

The index of an update comes from the epoch and the batch index (`position`), never from a counter of its own, so a resumed run continues
the schedule where the epoch it resumes at begins.
"""
import math

SCHEDULES = ('constant', 'cosine')


class LRSchedule:
    """lr(u) for the 0-based update index u of a run of `total_updates` updates:

      warmup   u < warmup_updates: base_lr * (u + 1) / warmup_updates -- base_lr / N at the first update, base_lr at the N-th;
      constant base_lr afterwards;
      cosine   from base_lr at the end of the warmup (update 0 without one) to lr_min at the LAST update:
               lr_min + (base_lr - lr_min) * (1 + cos(pi t)) / 2, t = (u - s) / (total_updates - 1 - s), s = max(warmup_updates - 1, 0).

    Param groups keep their proportions: every group's lr is its base value (`group_lrs`, read when the schedule is built) times
    factor(u) = lr(u) / base_lr.  ValueError: an unknown schedule, negative or non-integer counts, lr_min outside [0, base_lr].  A warmup longer than
    the run is allowed: the run ends inside the ramp."""

    def __init__(self, base_lr, total_updates, warmup_updates=0, schedule='constant', lr_min=0.0, group_lrs=None):
        if schedule not in SCHEDULES:
            raise ValueError(f'lr schedule {schedule!r}: expected one of {SCHEDULES}')
        for name, v in (('total_updates', total_updates), ('warmup_updates', warmup_updates)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 0:
                raise ValueError(f'invalid {name}: {v!r} (must be an integer >= 0)')
        for name, v in (('base_lr', base_lr), ('lr_min', lr_min)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
                raise ValueError(f'invalid {name}: {v!r} (must be a finite number >= 0)')
        if lr_min > base_lr:
            raise ValueError(f'lr_min = {lr_min!r} exceeds the learning rate {base_lr!r}')
        self.base_lr, self.total_updates, self.warmup_updates = float(base_lr), total_updates, warmup_updates
        self.schedule, self.lr_min = schedule, float(lr_min)
        self.group_lrs = None if group_lrs is None else [float(v) for v in group_lrs]

    @property
    def is_default(self):
        """No warmup and a constant rate: apply() changes nothing, and callers may skip it altogether."""
        return self.warmup_updates == 0 and self.schedule == 'constant'

    def lr(self, u):
        if isinstance(u, bool) or not isinstance(u, int) or u < 0:
            raise ValueError(f'invalid update index: {u!r} (must be an integer >= 0)')
        if u < self.warmup_updates:
            return self.base_lr * (u + 1) / self.warmup_updates
        if self.schedule == 'constant':
            return self.base_lr
        s = max(self.warmup_updates - 1, 0)
        t = min((u - s) / max(self.total_updates - 1 - s, 1), 1.0)
        return self.lr_min + (self.base_lr - self.lr_min) * 0.5 * (1.0 + math.cos(math.pi * t))

    def factor(self, u):
        return self.lr(u) / self.base_lr if self.base_lr > 0 else 1.0

    @staticmethod
    def updates_per_epoch(batches, accumulate=1):
        """Updates of an epoch of `batches` batches: one per `accumulate` batches, and one more for the batches left over (flush())."""
        return -(-batches // accumulate)

    @classmethod
    def position(cls, epoch, batch_index, batches, accumulate=1):
        """The 0-based index of the update that batch `batch_index` (0-based) of epoch `epoch` belongs to."""
        return epoch * cls.updates_per_epoch(batches, accumulate) + batch_index // accumulate

    def apply(self, step, u):
        """Set `step.lr` and every param group's lr for update u.  A default schedule touches nothing."""
        if self.is_default:
            return
        f = self.factor(u)
        step.lr = self.base_lr * f
        groups = getattr(step, 'param_groups', None)
        if groups is not None and self.group_lrs is not None:
            for g, base in zip(groups, self.group_lrs):
                g['lr'] = base * f
