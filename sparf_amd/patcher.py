"""Under the reference's names: the one patch-and-restore behind every `install*()` / `uninstall*()` pair of this package
(camera, losses, metrics, pose_eval).  Each pair owns one Patcher, so the pairs stay independent of one another."""


class Patcher:
    """The attributes one installer has replaced, and the originals it keeps for its hand-over paths."""

    def __init__(self, install, uninstall):
        """install: the dotted public name of the installer ("sparf_amd.losses.install_sampler"); uninstall: the bare name of its
        counterpart -- both only for the text of guard()"""
        self.message = f"{install}: already installed; call {uninstall}() first"
        self.patched, self.originals = [], {}

    def guard(self):
        if self.patched:
            raise RuntimeError(self.message)

    def put(self, obj, name, new):
        """obj.name = new until restore().  What is remembered is what `obj` itself held: a method living on a base class, or a
        function on an instance's class, is not in vars(obj), and restore() then deletes the attribute instead of writing it back."""
        self.patched.append((obj, name, name in vars(obj), vars(obj).get(name)))
        setattr(obj, name, new)

    def save(self, name, fn):
        """keep `fn` as original(name); the first one saved under a name stays"""
        self.originals.setdefault(name, fn)

    def original(self, name):
        """what save() kept under `name`, None without one"""
        return self.originals.get(name)

    def restore(self):
        """undo every put(), the last first, and forget the originals; a second call does nothing"""
        while self.patched:
            obj, name, own, old = self.patched.pop()
            if own:
                setattr(obj, name, old)
            else:
                delattr(obj, name)
        self.originals.clear()
