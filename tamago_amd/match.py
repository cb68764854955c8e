"""python -m tamago_amd.match: a match between two networks under Gumbel search (tamago_amd/selfplay/match.py) or, with
--search puct, under the PUCT search the GTP engine plays with (tamago_amd/selfplay/puct_match.py)."""
from tamago_amd.selfplay.match import main, parse_args, search_match   # noqa: F401

if __name__ == "__main__":
    main()
