from .._overlay import extend as _extend

_extend(__path__, "training")
