def chunked_vocoder_class(generator, lookahead=False):
    """The chunked class that plays ``generator`` (kantts.models.hifigan.chunked*), the one place that decides it.
    ``lookahead`` allows the non-causal classes, whose audio comes ``delay_samples`` late; without it a non-causal
    generator reaches a causal class and is refused there.  The class picked refuses, at construction, what nothing plays
    (non-causal multi-band: ``ChunkedMBVocoder``; multi-band NSF: ``ChunkedMBVocoder``)."""
    nsf, mb = bool(generator.nsf_enable), int(generator.out_channels) > 1
    if lookahead and not getattr(generator, "causal", False) and not mb:
        if nsf:
            from kantts.models.hifigan.chunked_nc_nsf import ChunkedNCNSFVocoder as cls
        else:
            from kantts.models.hifigan.chunked_nc import ChunkedNCVocoder as cls
    elif mb:
        from kantts.models.hifigan.chunked_mb import ChunkedMBVocoder as cls
    elif nsf:
        from kantts.models.hifigan.chunked_nsf import ChunkedNSFVocoder as cls
    else:
        from kantts.models.hifigan.chunked import ChunkedVocoder as cls
    return cls
