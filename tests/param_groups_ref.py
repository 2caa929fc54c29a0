"""float64 restatement of the grouped update (include/bidate_hip.h bdn_*_step_grouped): tests/optim_ref.py's rules applied segment by
segment.  Shared by tests/test_param_groups_cpu.py (which pins it against CPU torch.optim with the same groups) and
tests/test_gpu_param_groups.py (which holds the HIP kernels to it)."""
import torch

from fabric_amd.optim import FROZEN

from tests import optim_ref as R


def grouped_reference(kind, rule, segs, hyper, p, g, state, step, grad_scale=1.0):
    """tests/optim_ref.py's sgd / adam applied segment by segment.  segs: [(start, stop, group id)] in elements; hyper: per group
    (lr, weight_decay); state: {'buf'} or {'m', 'v'} (float32, not modified).  -> ({name: (value, magnitude)}) over the whole buffers
    in float64, with frozen segments carrying the inputs themselves and magnitude 0 (any change at all is an error)."""
    out = {'p': (p.double().clone(), torch.zeros_like(p, dtype=torch.float64))}
    for key in state:
        out[key] = (state[key].double().clone(), torch.zeros_like(p, dtype=torch.float64))
    for a, b, gid in segs:
        if gid == FROZEN:
            continue
        lr, wd = hyper[gid]
        sl = slice(a, b)
        if kind == 'sgd':
            mom = rule.get('momentum', 0.0)
            rp, rb, mp, mb = R.sgd(p[sl], g[sl], state['buf'][sl] if mom else None, lr, grad_scale, mom, rule.get('dampening', 0.0), wd,
                                   rule.get('nesterov', False), first=step == 1)
            res = {'p': (rp, mp)}
            if mom:
                res['buf'] = (rb, mb)
        else:
            rp, rm, rv, mp, mm, mv = R.adam(p[sl], g[sl], state['m'][sl], state['v'][sl], step, lr, grad_scale,
                                            rule.get('betas', (0.9, 0.999)), rule.get('eps', 1e-8), wd, kind == 'adamw')
            res = {'p': (rp, mp), 'm': (rm, mm), 'v': (rv, mv)}
        for key, (val, mag) in res.items():
            out[key][0][sl] = val
            out[key][1][sl] = mag
    return out
