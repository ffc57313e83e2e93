"""CPU: the matchup-evaluation entry points exist and refuse a NULL handle; the ABI
version did not move; the CLI has the tournament flags, off by default."""
import ctypes

import pytest

from maddpg_amd import _lib

NAMES = ("mdp_actor_set_floats", "mdp_actor_set_write", "mdp_actor_set_snapshot", "mdp_evaluate_matchups")


def test_library_exports_the_matchup_entry_points():
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name in _lib.header_symbols(), name
    # a NULL handle is refused (no launch, no crash)
    assert lib.mdp_actor_set_floats(None) == -1
    src = (ctypes.c_float * 8)()
    assert lib.mdp_actor_set_write(None, None, 0, src, 8) < 0
    assert lib.mdp_actor_set_snapshot(None, None) < 0
    table = (ctypes.c_int32 * 3)()
    assert lib.mdp_evaluate_matchups(None, None, 1, table, 1, 0, 16, 0, None, None, None) < 0
    # entry points were added and none changed: the ABI version and the timed kinds stay
    assert lib.mdp_abi_version() == _lib.ABI_VERSION == 5
    text = open(_lib.HEADER).read()
    assert "MDP_K_EVAL = 12" in text and "MDP_K_COUNT = 13" in text
    assert _lib.EVAL_MAX_SETS == 4096 and _lib.EVAL_MAX_MATCHUP_EPISODES == 1 << 22


def test_cli_has_the_tournament_flags_off_by_default():
    from experiments.train import parse_args
    a = parse_args([])
    assert a.tournament == [] and a.tournament_team == ""
    b = parse_args(["--evaluate", "--tournament", "/x/", "/y/", "--tournament-team", "0,2"])
    assert b.evaluate and b.tournament == ["/x/", "/y/"] and b.tournament_team == "0,2"


def _args(**kw):
    base = dict(tournament=["/x/", "/y/"], tournament_team="", evaluate=True, adv_load_dir="", num_adversaries=3)
    base.update(kw)
    return type("Args", (), base)()


def test_tournament_flag_combinations_are_refused_with_a_message():
    from experiments.train import tournament_team
    assert tournament_team(_args(), 4) == [0, 1, 2]
    assert tournament_team(_args(tournament_team="3,1"), 4) == [1, 3]
    with pytest.raises(SystemExit, match="--tournament needs --evaluate"):
        tournament_team(_args(evaluate=False), 4)
    with pytest.raises(SystemExit, match="--adv-load-dir"):
        tournament_team(_args(adv_load_dir="/z/"), 4)
    with pytest.raises(SystemExit, match="empty"):
        tournament_team(_args(num_adversaries=0), 4)
    with pytest.raises(SystemExit, match="every agent"):
        tournament_team(_args(tournament_team="0,1,2,3"), 4)
    with pytest.raises(SystemExit, match="every agent"):
        tournament_team(_args(num_adversaries=9), 4)
    with pytest.raises(SystemExit, match="out of range"):
        tournament_team(_args(tournament_team="0,4"), 4)
    with pytest.raises(SystemExit, match="agent indices"):
        tournament_team(_args(tournament_team="a,b"), 4)
