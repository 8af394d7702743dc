"""Test infrastructure: the library behind a proxy that notes the name of every entry point called through it.  Put in
``engine.L`` of an Arena or League (they look it up when a match starts), it gives the match's sequence of library calls."""


class Calls:

    def __init__(self, L):
        self._L, self.names = L, []

    def __getattr__(self, name):
        fn = getattr(self._L, name)

        def call(*args):
            self.names.append(name)
            return fn(*args)
        return call
