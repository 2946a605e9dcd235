"""Learning-rate schedules for the four train() loops: what `--scheduler-type`, `--lr-step-size` and `--lr-gamma` of
train_cae select.  Host arithmetic only (python floats, no torch): the engines take the resulting rate through set_lr().

The semantics are those of the torch.optim.lr_scheduler classes the flag help names, with the flags mapped as

    StepLR             StepLR(step_size=lr_step_size, gamma=lr_gamma)
    ExponentialLR      ExponentialLR(gamma=lr_gamma)
    CosineAnnealingLR  CosineAnnealingLR(T_max=lr_step_size, eta_min=0), periodic past T_max as torch's recursion is
    ReduceLROnPlateau  ReduceLROnPlateau(mode="min", factor=lr_gamma, patience=lr_step_size), torch's other defaults

The first three are stepped once after every training epoch (step()); the plateau schedule is stepped with the test loss
at each epoch where the test pass runs (step_metric()).  `wants_metric` says which of the two a schedule listens to; the
other call is a no-op, so a loop may call both unconditionally.
"""
import math

SCHEDULER_TYPES = ("StepLR", "ReduceLROnPlateau", "ExponentialLR", "CosineAnnealingLR")


def is_constant(scheduler_type):
    """None, "" and the literal string "None" (what a driver that always passes the flag sends) mean no schedule"""
    return scheduler_type is None or scheduler_type in ("", "None")


def check_scheduler_type(scheduler_type):
    """the name as make_schedule() will read it (None for a constant rate); ValueError for an unknown one"""
    if is_constant(scheduler_type):
        return None
    if scheduler_type not in SCHEDULER_TYPES:
        raise ValueError(f"unknown scheduler type {scheduler_type!r}: expected one of {', '.join(SCHEDULER_TYPES)} "
                         "(or None for a constant learning rate)")
    return scheduler_type


class ConstantLR:
    """no schedule: the rate the optimiser was created with"""

    active = False
    wants_metric = False

    def __init__(self, base_lr):
        self.base_lr = self.lr = float(base_lr)
        self.last_epoch = 0

    def step(self):
        pass

    def step_metric(self, value):
        pass


class _EpochSchedule(ConstantLR):
    active = True

    def step(self):
        self.last_epoch += 1
        self.lr = self._next()


class StepLR(_EpochSchedule):
    """multiplied by gamma after every step_size epochs (torch applies the factor to the running value)"""

    def __init__(self, base_lr, step_size, gamma):
        super().__init__(base_lr)
        self.step_size, self.gamma = int(step_size), float(gamma)
        if self.step_size < 1:
            raise ValueError(f"StepLR: lr_step_size must be a positive number of epochs, got {step_size}")

    def _next(self):
        return self.lr * self.gamma if self.last_epoch % self.step_size == 0 else self.lr


class ExponentialLR(_EpochSchedule):
    """multiplied by gamma after every epoch"""

    def __init__(self, base_lr, gamma):
        super().__init__(base_lr)
        self.gamma = float(gamma)

    def _next(self):
        return self.lr * self.gamma


class CosineAnnealingLR(_EpochSchedule):
    """base_lr * (1 + cos(pi * epoch / T_max)) / 2: down to 0 at T_max and, like torch's recursion, back up and down again with
    period 2 * T_max beyond it.  The closed form: it passes through 0 where the recursion leaves about 1e-18."""

    def __init__(self, base_lr, t_max):
        super().__init__(base_lr)
        self.t_max = int(t_max)
        if self.t_max < 1:
            raise ValueError(f"CosineAnnealingLR: lr_step_size (T_max) must be a positive number of epochs, got {t_max}")

    def _next(self):
        # the epoch is folded into one period first, so that cos() sees the same small argument in every period
        e = self.last_epoch % (2 * self.t_max)
        return self.base_lr * (1.0 + math.cos(math.pi * e / self.t_max)) / 2.0


class ReduceLROnPlateau(ConstantLR):
    """multiplied by `factor` once the metric has failed to improve on the best value seen, by more than the relative
    threshold, for more than `patience` steps in a row (torch's mode="min", threshold_mode="rel", cooldown=0, min_lr=0)"""

    active = True
    wants_metric = True
    THRESHOLD = 1e-4
    EPS = 1e-8      # a reduction smaller than this is not applied

    def __init__(self, base_lr, patience, factor):
        super().__init__(base_lr)
        self.patience, self.factor = int(patience), float(factor)
        if self.factor >= 1.0:
            raise ValueError("ReduceLROnPlateau: lr_gamma (the factor) must be below 1.0")
        self.best = math.inf
        self.num_bad_epochs = 0

    def step_metric(self, value):
        value = float(value)
        self.last_epoch += 1
        if value < self.best * (1.0 - self.THRESHOLD):
            self.best = value
            self.num_bad_epochs = 0
        else:
            self.num_bad_epochs += 1
        if self.num_bad_epochs > self.patience:
            new_lr = max(self.lr * self.factor, 0.0)
            if self.lr - new_lr > self.EPS:
                self.lr = new_lr
            self.num_bad_epochs = 0


def make_schedule(scheduler_type, base_lr, step_size=500, gamma=0.5):
    """the schedule `scheduler_type` names, starting at base_lr: an object with `lr` (the current rate), `step()`,
    `step_metric(value)`, `wants_metric` and `active` (False for the constant rate)"""
    kind = check_scheduler_type(scheduler_type)
    if kind is None:
        return ConstantLR(base_lr)
    if kind == "StepLR":
        return StepLR(base_lr, step_size, gamma)
    if kind == "ExponentialLR":
        return ExponentialLR(base_lr, gamma)
    if kind == "CosineAnnealingLR":
        return CosineAnnealingLR(base_lr, step_size)
    return ReduceLROnPlateau(base_lr, step_size, gamma)
