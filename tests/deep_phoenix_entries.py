"""The two deep Phoenix entry points as the footprint tests call them: fr_render_deep_phoenix with an fp64 view and
fr_render_deepx_phoenix with an extended one, through the renderer and through the C function."""
import ctypes as C


class Entry:
    """name: the entry point less "fr_render_"; view: a view of deep_phoenix_ref / deepx_phoenix_ref; sizes: the frames its test
    renders; where the zoom travels (state_kw: in the state, view_kw: in the view, as a string) and how the view becomes a C
    struct (to_c); bla_kw, flag: what switches its iteration skipping on, for the renderer and in fr_params.flags"""

    def __init__(self, name, view, sizes, state_kw, view_kw, to_c, bla_kw, flag):
        self.name, self.view, self.sizes = name, view, sizes
        self.state_kw, self.view_kw, self.to_c, self.bla_kw, self.flag = state_kw, view_kw, to_c, bla_kw, flag

    def __repr__(self):
        return self.name

    def state(self, fr):
        return fr.FractalState(max_iterations=self.view["max_iter"], **self.state_kw)

    def deep_view(self, fr):
        return fr.DeepView(self.view["cx"], self.view["cy"], **self.view_kw)

    def ph(self, fr):
        return fr.PhoenixParams(phoenix_p=self.view["p"], phoenix_r=self.view["r"])

    def render(self, fr, renderer, W, H, **kw):
        getattr(renderer, "render_" + self.name)(self.state(fr), W, H, self.deep_view(fr), self.ph(fr), **kw)

    def render_c(self, fr, renderer, W, H, shard, out, flags=0):
        """the C function on one part of a sharding; returns its status"""
        p = self.state(fr).to_params(fr.FractalType.Phoenix, fr.Precision.F64, False)
        p.flags |= flags
        cv = getattr(self.deep_view(fr), self.to_c)()
        ph = self.ph(fr).to_c()
        sh = shard.to_c()
        return getattr(fr.lib(), "fr_render_" + self.name)(renderer._ctx, C.byref(p), C.byref(ph), C.byref(cv), W, H, C.byref(sh),
                                                           C.byref(out))

    def last_steps(self, renderer):
        return tuple(getattr(renderer, "last_" + self.name + "_steps")())


def fp64(view, sizes):
    return Entry("deep_phoenix", view, sizes, {"zoom": view["zoom"]}, {}, "to_c", {"bla": True}, "FR_FLAG_DEEP_PHOENIX_BLA")


def extended(view, sizes):
    return Entry("deepx_phoenix", view, sizes, {}, {"zoom": view["zoom"]}, "to_cx", {"xbla": True}, "FR_FLAG_DEEPX_PHOENIX_BLA")


def cases(entries, first=0):
    """(entry, size) over every entry's own sizes from `first` on, for pytest.mark.parametrize("entry,geom", ...)"""
    return [(e, g) for e in entries for g in e.sizes[first:]]


def case_id(v):
    return "%dx%d" % v if isinstance(v, tuple) else repr(v)
