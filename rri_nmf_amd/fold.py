"""The one-launch fold sweep of a pattern-only handle (include/rri_fold.h): functions that take an RRIEngine.

    set_fold_schedule(engine, on=True)   ask a weighted='sparse' handle for the schedule (or take the request back)
    fold_info(engine)                    what was asked, whether it applies, and how the handle's sweeps were taken

With T fixed the W half of a sweep touches a row of W through that row's own observed entries alone, and a handle that asked takes
it as one launch per sweep (k <= 64, one device) where the launch-per-topic schedule takes about four per topic.  Opt-in and per
handle: a handle that never asks sweeps exactly as before.  nmf(..., fold_in=True) asks for the call's handle, and
NMF_RS_Estimator.transform_corpus folds new users in from a DeviceCorpus that way.

They are functions, not methods: the entry points are declared in a header of their own and typed from a table of their own
(_capi.FOLD_PROTOTYPES).
"""
import ctypes as C

FOLD_INFO_FIELDS = ('asked', 'eligible', 'launches', 'stepped', 'halts', 'rows_per_group')
FOLD_MAX_K = 64     # rri_fold.hpp: a larger rank runs launch by launch, and fold_info says so


def set_fold_schedule(engine, on=True):
    """Ask the handle for the one-launch W half of sweeps with T fixed (rri_set_fold_schedule); on=False takes the request back.
    Remembered for the handle's life; touches no cached state.  A handle that is not weighted='sparse' is refused (ValueError)."""
    engine._check(engine._lib.rri_set_fold_schedule(engine._h, 1 if on else 0))


def fold_info(engine):
    """rri_fold_info as a dict: asked, eligible (under the parameters set last), launches (sweeps taken as one launch), stepped
    (sweeps that ran launch by launch while asked), halts (found inside a launch), rows_per_group."""
    out = (C.c_int64 * 6)()
    engine._check(engine._lib.rri_fold_info(engine._h, out))
    info = dict(zip(FOLD_INFO_FIELDS, (int(v) for v in out)))
    info['asked'], info['eligible'] = bool(info['asked']), bool(info['eligible'])
    return info


__all__ = ['set_fold_schedule', 'fold_info', 'FOLD_MAX_K']
