"""CPU: the reference's own search vectors (mcts_test.cc, tests/mcts_known_answers.py) on the CPU restatement of the search and --
where oracle/_ref is present -- on the reference's self-play stack (the stand-in build)."""
import pytest

import mcts_known_answers as mka
from pyoracle import RefSelfPlay


@pytest.mark.parametrize("case", mka.ALL_CASES, ids=lambda f: f.__name__)
def test_known_answer_on_the_restatement(built, case):
    case(mka.port_engine)


@pytest.mark.parametrize("case", mka.ALL_CASES, ids=lambda f: f.__name__)
def test_known_answer_on_the_reference_stack(built, case):
    if not RefSelfPlay.available(9):
        pytest.skip("oracle/_ref not built (no /root/reference here)")
    case(mka.ref_engine)
