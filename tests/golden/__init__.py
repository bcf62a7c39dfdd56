"""Golden vectors recorded from the real reference, and the scripts that made them (each script's docstring has its
command line).  ``ttt_transitions.npz`` -- the reference's TicTacToe over the whole game -- is regenerated with

    PYTHONPATH=/root/reference/src PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_ttt_transitions.py

which asserts the row counts (4 520 positions, 16 167 (position, action) pairs, 46 506 rows) before it writes."""
