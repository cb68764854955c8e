"""python -m tamago_amd.tournament: a round robin between networks under strict PUCT search, every game of every pairing in one
lock-step engine (tamago_amd/selfplay/tournament.py)."""
from tamago_amd.selfplay.tournament import main, parse_args, puct_tournament   # noqa: F401

if __name__ == "__main__":
    main()
