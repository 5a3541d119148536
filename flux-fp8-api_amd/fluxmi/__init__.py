class GenerationCancelled(RuntimeError):
    """A request stopped by its `on_step` callback (FluxPipeline.generate) or step hook (Flux.denoise): `evaluations` = the model
    evaluations that ran before the engine stopped launching, `num_evaluations` = what the whole request would have run."""

    def __init__(self, evaluations: int, num_evaluations: int):
        super().__init__(f"fluxmi: generation cancelled after {evaluations} of {num_evaluations} model evaluations")
        self.evaluations = int(evaluations)
        self.num_evaluations = int(num_evaluations)
