"""Proof backup, MCTS-Solver (az_engine_set_proof_backup): the option's form, checked where it is given.  The option
is a bool: with it on, a node of the search tree is proven as soon as its children decide it, proven nodes are not searched again, and
the move and the policy target respect the proofs.  It combines with exact endgames; which search modes serve it is the engine's to
check, and is checked here before any device work."""
import numpy as np


def parse(spec, name="proof_backup"):
    """bool of a checked spec (None: off); ValueError naming `name` otherwise"""
    if spec is None:
        return False
    if not isinstance(spec, (bool, np.bool_)):
        raise ValueError(f"{name}={spec!r}: expected a bool (True: proven wins, losses and draws are backed up the search tree)")
    return bool(spec)


def check_combination(spec, name, others):
    """`others`: {option name: value} of the modes proof backup does not combine with (None / 1 / False = off); ValueError naming both"""
    on = parse(spec, name)
    if not on:
        return False
    for oname, val in others.items():
        if val is not None and val is not False and val != 1:
            raise ValueError(f"{name}={spec!r} does not combine with {oname}={val!r}: proof backup is served in the plain PUCT search "
                             f"only (one leaf per lock-step, no playout cap, no forced playouts; exact endgames combine with it)")
    return True


def check_proof_backup(spec, nn=None, symmetry=None, leaf_batch=None, gumbel=None, neural=True, name="proof_backup"):
    """whether `spec` switches the mode on; ValueError -- before any device work -- for a malformed one, for a rollout-mode tree, for a
    network that evaluates its leaves through an external evaluator (evaluators.route), and next to symmetry, leaf_batch > 1 or gumbel"""
    if not check_combination(spec, name, {"symmetry": symmetry, "leaf_batch": leaf_batch, "gumbel": gumbel}):
        return False
    if not neural:
        raise ValueError(f"{name}={spec!r} needs eval_method 'neural': a rollout tree (random playouts) is not served by proof backup")
    if nn is not None:
        from .evaluators import route
        if route(nn) != "hip":
            raise ValueError(f"{name}={spec!r} needs a network the HIP network serves; {type(nn).__name__} evaluates its leaves through "
                             f"an external evaluator, which proof backup is not served for")
    return True
