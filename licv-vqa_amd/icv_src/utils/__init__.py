"""Mirror of the reference's ``icv_src.utils`` for the part the ICL baseline needs: the RICE retriever."""
