"""The stop-and-go walk of checkpointed Model.solve_many / Model.resume_many in their terms (a helper module of
test_many_resume_host.py and test_gpu_many_resume.py, no test itself): many_walk.Walk with the objective fixed when it
is made, its results in many_walk.dive()'s form."""
import many_walk
from many_walk import BAD_ROOT, DONE, LIMIT  # noqa: F401


class Walk(many_walk.Walk):
    def __init__(self, text, root_row, objective="ANY"):
        assert objective in ("ANY", "ALL")
        super().__init__(text, root_row)
        self.stop_at = 1 if objective == "ANY" else None

    def result(self):
        return many_walk.first_of(super().result())

    def run(self, budget):
        """at most `budget` more children -> the counters so far (status LIMIT: stopped with work left)"""
        return super().run(budget, self.stop_at)


def solutions_below(text, states):
    """solutions of the ALL trees below `states`: each propagated as a root row, then walked; a state that is a solution
    after propagation counts one (dive() does exactly this with a root row)"""
    return sum(many_walk.dive(text, s, "ALL")["solutions"] for s in states)
