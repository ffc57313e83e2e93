"""The training variants as the Python layers see them.

maddpg_amd/csrc/mdp_variants.h is the table the library decides by; this is
the same table for what refuses before a handle exists: Engine's and
VecRunner's keyword checks and the flag checks of experiments/train.py.  No
two rows combine, and none runs in throughput mode or on several GPUs.  A new
variant is one row here and one there.  Nothing heavy is imported: the CLI
checks its flags before torch or the library load.
"""
from collections import namedtuple

# kw: the Engine / VecRunner keyword; flag: the CLI's; npz_only: its checkpoints
# have state without reference variable names, so no TF1 bundle; precheck: the
# CLI and VecRunner refuse its combinations themselves (prioritized replay
# predates those checks: the library's own refusal is what its callers see)
Row = namedtuple("Row", "kw flag name npz_only precheck")

VARIANTS = (
    Row("prioritized", "--prioritized-replay", "prioritized replay", False, False),
    Row("td3", "--td3", "MATD3", True, True),
    Row("minimax", "--minimax", "M3DDPG", False, True),
    Row("approx", "--approx-policies", "inferred policies", True, True),
)
# not a variant but a property of the action spaces, with the same exclusions
BOX = Row("continuous", "--continuous-actions", "Box action spaces", False, True)
ROWS = VARIANTS + (BOX,)


def dest(row):
    """the argparse attribute of the row's flag"""
    return row.flag.lstrip("-").replace("-", "_")


def by_flag(flag):
    return next(r for r in ROWS if r.flag == flag)


def engine_refusal(asked, world_size=1):
    """why an Engine asked for the variants `asked` ({kw: bool}) on `world_size`
    GPUs cannot be built, or None"""
    on = [r for r in VARIANTS if asked.get(r.kw)]
    if len(on) > 1:
        return f"{on[0].name} ({on[0].kw}) and {on[1].name} ({on[1].kw}) do not combine: one variant per handle"
    if on and world_size > 1:
        return f"{on[0].name} ({on[0].kw}) runs on one GPU: no data-parallel exchange (world_size {world_size})"
    return None


def runner_refusal(asked, world_size=1):
    """why a VecRunner with the keywords `asked` cannot span `world_size` GPUs, or None"""
    for r in ROWS:
        if r.precheck and asked.get(r.kw) and world_size > 1:
            return f"{r.flag} runs on one GPU ({r.name}: no data-parallel variant)"
    return None


def flag_refusal(flag, arglist, world=1):
    """why the command line `arglist` (an argparse namespace; an attribute it
    lacks counts as not given) cannot have `flag`, or None.  The three wordings
    are the CLI's own: a second flag, the update mode, the GPU count."""
    me = by_flag(flag)
    if not getattr(arglist, dest(me), False):
        return None
    for r in ROWS:
        if r is not me and getattr(arglist, dest(r), False):
            return f"{flag} does not combine with {r.flag}"
    if getattr(arglist, "update_mode", "strict") != "strict":
        return f"{flag} needs --update-mode strict"
    if (getattr(arglist, "num_gpus", None) or 1) > 1 or world > 1:
        return f"{flag} runs on one GPU (--num-gpus 1)"
    if me.npz_only and getattr(arglist, "save_format", "npz") == "tf1":
        return f"{flag} saves npz checkpoints only ({me.name}: state without reference variable names)"
    return None
